"""Polyphony on the device (csrc/ddsp_voices.hip): the cases of tests/test_voices_host.py on `cuda`
against the plain loops of tests/voices_reference.py -- the allocation to the bit, the mix within (V + 6) 2^-24 of the sum of
the terms' magnitudes --, more rows than the allocation's grid, guard zones around every output of both entry points, graph
replay, and `AutoEncoder.play(notes, voices=V)`."""
import numpy as np
import pytest
import torch

import ddsp_pytorch_amd as ddsp
import voices_reference as vref
from ddsp_pytorch_amd import voices
from ddsp_pytorch_amd.notes import Notes
from encoder_common import AEConf
from test_voices_host import (EXTRA_MIX, GATES, HOP, MIX_SHAPES, RECORDS, VOICE_KEYS, bits, check_alloc, check_designed_allocation, check_mix,
                              check_one_voice_renders_as_the_source, check_ungated_single_voice_is_a_copy, got_alloc, mix_case, notes_of,
                              random_score, run_mix, run_random_allocation, want_alloc)

pytestmark = pytest.mark.gpu
GUARD = 51                                                      # fits every output type


def guarded(n, dtype, pad=64):
    whole = torch.full((n + 2 * pad,), GUARD, device="cuda", dtype=dtype)
    return whole, whole[pad:pad + n]


def guards_intact(whole, n, pad=64):
    return bool((whole[:pad] == GUARD).all()) and bool((whole[pad + n:] == GUARD).all())


def test_device_allocation_equals_plain_loops():
    run_random_allocation("cuda")


def test_designed_scores_fire_every_rule_on_the_device():
    check_designed_allocation("cuda")
    check_one_voice_renders_as_the_source("cuda")


def test_more_rows_than_the_grid():
    """2051 rows of 5 notes on 3 voices: more rows than the 2048 workgroups the kernel strides over, every one checked against the
    CPU path (which tests/test_voices_host.py pins to the loops) and a few against the loops themselves"""
    B, N, V = 2051, 5, 3
    rec = random_score(9, B=B, N=N)
    rec["onset"][:] = np.cumsum(np.random.default_rng(10).integers(0, 3, (B, N)), axis=1)
    for steal in ("oldest", "quietest"):
        got = got_alloc(rec, "cuda", V, N, "nearest", steal, 1)
        check_alloc(got, got_alloc(rec, "cpu", V, N, "nearest", steal, 1), ("2051 rows", steal))
        rows = [0, 1, 2, 2046, 2047, 2048, 2049, 2050]
        want = want_alloc({k: v[rows] for k, v in rec.items()}, V, N, "nearest", steal, 1)
        voice_rows = [b * V + v for b in rows for v in range(V)]
        part = {k: got[k][voice_rows if got[k].shape[0] == B * V else rows] for k in VOICE_KEYS}
        check_alloc(part, want, ("2051 rows, against the loops", steal))
        assert int(got["stolen"].sum()) > 500 and int((got["count"] == 0).sum()) > 0


def raw_allocate(rec, outs, B, N, V, Nv, assign, steal, gap):
    src = [torch.from_numpy(rec[k]).cuda() for k in RECORDS]
    count = torch.from_numpy(rec["count"]).cuda()
    ptr = lambda x: x.data_ptr() if x.numel() else None           # noqa: E731
    return ddsp._lib.lib().ddsp_voices_allocate(*(ptr(x) for x in src), count.data_ptr(), *(ptr(outs[k]) for k in RECORDS), ptr(outs["count"]),
                                                ptr(outs["index"]), ptr(outs["voice"]), ptr(outs["slot"]), ptr(outs["stats"]), B, N, V, Nv,
                                                vref.ASSIGN[assign], vref.STEAL[steal], gap, torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("N,Nv", [(12, 12), (12, 2), (12, 0), (0, 4), (70, 3)])
def test_allocation_guard_zones_and_overflow(N, Nv):
    """guard zones around every output; with Nv below a voice's count nothing is written past Nv and the count still counts;
    N = 0 and Nv = 0 write their fills and counts only"""
    B, V = 5, 3
    rec = random_score(31, B=B, N=N)
    sizes = dict({k: B * V * Nv for k in RECORDS + ("index",)}, count=B * V, voice=B * N, slot=B * N, stats=2 * B)
    wholes = {k: guarded(n, torch.float32 if k == "level" else torch.int32) for k, n in sizes.items()}
    want = want_alloc(rec, V, Nv, "oldest", "quietest", 0)
    for _ in range(2):                                          # a second run gives equal bits
        assert raw_allocate(rec, {k: o for k, (_, o) in wholes.items()}, B, N, V, Nv, "oldest", "quietest", 0) == 0
        torch.cuda.synchronize()
        assert all(guards_intact(wholes[k][0], n) for k, n in sizes.items())
        got = {k: wholes[k][1].cpu().numpy().reshape(want[k].shape) for k in sizes if k != "stats"}
        stats = wholes["stats"][1].cpu().numpy().reshape(B, 2)
        check_alloc(dict(got, stolen=stats[:, 0], dropped=stats[:, 1]), want, ("guarded", N, Nv))
    if N:
        assert (want["count"] > Nv).any() if Nv < 4 else (want["count"] <= Nv).all()


@pytest.mark.parametrize("V,C,L", MIX_SHAPES)
def test_device_mix_is_within_its_derived_bound(V, C, L):
    for gate in GATES:
        run_mix(V, C, L, gate, "cuda")


@pytest.mark.parametrize("V,C,L,gate,hop", EXTRA_MIX)
def test_device_mix_over_tiles_small_hops_and_long_look_backs(V, C, L, gate, hop):
    got = run_mix(V, C, L, gate, "cuda", hop)
    again = run_mix(V, C, L, gate, "cuda", hop)
    assert torch.equal(got, again)


def test_device_mix_of_one_voice_without_a_gate_copies_the_bits():
    check_ungated_single_voice_is_a_copy("cuda")


@pytest.mark.parametrize("V,C,L,gate,hop", [(3, 2, 67, GATES[3], HOP), (3, 1, 1, GATES[2], HOP), (64, 2, 4 * 172 + 3, None, HOP),
                                            (3, 2, 2052, None, HOP), (3, 1, 2052, GATES[3], HOP), (2, 2, 700, (70, 30, "above"), 5)])
def test_mix_guard_zones(V, C, L, gate, hop):
    case = mix_case(V, C, L, gate, hop)
    B = case["B"]
    audio, table = torch.from_numpy(case["audio"]).cuda(), torch.from_numpy(case["table"]).cuda()
    active = None if case["active"] is None else torch.from_numpy(case["active"]).cuda().view(torch.uint8)
    whole, out = guarded(B * C * L, torch.float32)              # (the guard puts `out` off 16-byte alignment only if pad were odd: 64 floats)
    T = 0 if active is None else active.shape[1]
    rc = ddsp._lib.lib().ddsp_voices_mix(audio.data_ptr(), table.data_ptr(), None if active is None else active.data_ptr(), out.data_ptr(), B, V,
                                         C, L, T, hop if active is not None else 0, case["hold"], case["fade"], torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert guards_intact(whole, B * C * L)
    check_mix(out.cpu().numpy(), case, V, ("guarded", V, C, L, gate, hop))


def test_unaligned_rows_take_the_narrow_path():
    """audio and out that begin 4 bytes off a 16-byte boundary, with L a multiple of 4: the same values as the aligned call"""
    case = mix_case(3, 2, 2052, None, HOP)
    B, V, L = case["B"], 3, 2052
    table = torch.from_numpy(case["table"]).cuda()
    src = torch.zeros(B * V * L + 1, device="cuda")
    src[1:] = torch.from_numpy(case["audio"]).cuda().reshape(-1)
    whole, out = guarded(B * 2 * L, torch.float32, pad=65)
    rc = ddsp._lib.lib().ddsp_voices_mix(src[1:].data_ptr(), table.data_ptr(), None, out.data_ptr(), B, V, 2, L, 0, 0, 0, 0,
                                         torch.cuda.current_stream().cuda_stream)
    assert rc == 0 and src[1:].data_ptr() % 16 == 4 and out.data_ptr() % 16 == 4
    torch.cuda.synchronize()
    assert guards_intact(whole, B * 2 * L, pad=65)
    aligned = voices.mix_voices(torch.from_numpy(case["audio"]).cuda(), V, gain=case["gain"], pan=case["pan"])
    assert torch.equal(out.view(B, 2, L), aligned)


def test_graph_replay_on_changed_inputs_equals_eager():
    B, N, V, T = 3, 40, 4, 12
    L = T * HOP - 5
    recs = [random_score(61), random_score(62), random_score(63)]
    rng = np.random.default_rng(64)
    audios = [torch.from_numpy(rng.standard_normal((B * V, L)).astype(np.float32)).cuda() for _ in recs]
    actives = [torch.from_numpy(rng.random((B * V, T, 1)) < 0.3).cuda() for _ in recs]
    gain, pan = torch.from_numpy(rng.standard_normal((B, V))).cuda(), torch.from_numpy(rng.uniform(-1, 1, (V,))).cuda()
    notes, audio, active = notes_of(recs[0], "cuda"), audios[0].clone(), actives[0].clone()

    def launch():
        found, info = voices.allocate_voices(notes, V, steal="quietest", gap=1, max_notes=12, return_info=True)
        return found, info, voices.mix_voices(audio, V, gain=gain, pan=pan, active=active, hop_length=HOP, hold=1, fade=3)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()                                                # warm-up on the capture stream
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            found, info, mixed = launch()
    torch.cuda.current_stream().wait_stream(side)
    for rec, x, on in zip(recs[1:], audios[1:], actives[1:]):
        for k in RECORDS + ("count",):
            getattr(notes, k).copy_(torch.from_numpy(rec[k]))
        audio.copy_(x)
        active.copy_(on)
        found.pitch.fill_(-9)
        mixed.fill_(-9.0)
        graph.replay()
        torch.cuda.synchronize()
        e_found, e_info = voices.allocate_voices(notes_of(rec, "cuda"), V, steal="quietest", gap=1, max_notes=12, return_info=True)
        for k in RECORDS + ("count",):
            assert np.array_equal(bits(getattr(found, k).cpu().numpy()), bits(getattr(e_found, k).cpu().numpy())), k
        for k in e_info:
            assert torch.equal(info[k], e_info[k]), k
        eager = voices.mix_voices(x, V, gain=gain, pan=pan, active=on, hop_length=HOP, hold=1, fade=3)
        assert np.array_equal(bits(mixed.cpu().numpy()), bits(eager.cpu().numpy()))
        assert int(e_info["stolen"].sum()) > 3 and float(eager.abs().max()) > 0


def test_autoencoder_plays_chords():
    """play(notes, voices=V): within the mix's bound of the torch sum of the B V voice rows played unmixed through play; with the
    gate, the bits of mix_voices on those rows; and not what the monophonic play gives"""
    ae = ddsp.AutoEncoder(AEConf, tracker='yin').cuda().eval()
    hop, V, T = ae.hop_length, 3, 14
    chords = Notes(onset=[[0, 0, 0, 6, 6, 6], [1, 1, 1, 7, 7, 8]], frames=[[6, 6, 8, 6, 6, 6], [5, 5, 5, 6, 6, 5]],
                   pitch=[[60, 64, 67, 62, 65, 69], [57, 60, 64, 55, 59, 62]], level=[[0.8, 0.6, 0.7, 0.9, 0.5, 0.6], [0.7] * 6]).to("cuda")
    options = dict(attack=1, release=2)
    with torch.no_grad():
        rows, info = voices.allocate_voices(chords, V, return_info=True)
        assert int(info["dropped"].sum()) == 0 and bool((info["voice"] >= 0).all()) and rows.rows == 6
        torch.manual_seed(11)
        unmixed = ae.play(rows, frames=T, **options)
        torch.manual_seed(11)
        got = ae.play(chords, frames=T, voices=V, **options)
        torch.manual_seed(11)
        mono = ae.play(chords, frames=T, **options)
        assert got.shape == (2, T * hop) == mono.shape and unmixed.shape == (6, T * hop) and bool(torch.isfinite(got).all())
        want = unmixed.double().view(2, V, -1).sum(1)
        bound = vref.roundings(V) * 2.0 ** -24 * unmixed.double().abs().view(2, V, -1).sum(1)
        assert bool(((got.double() - want).abs() <= bound).all()) and float(got.abs().max()) > 0
        assert not torch.allclose(got, mono, atol=1e-4)
        # the gate and a pan: the same rows through mix_voices
        mix = dict(gate=True, hold=1, fade=2, pan=[-0.5, 0.0, 0.5], gain=[1.0, 0.5, 0.25])
        torch.manual_seed(11)
        gated = ae.play(chords, frames=T, voices=V, voice_options=dict(assign="lowest"), mix_options=mix, **options)
        lowest = voices.allocate_voices(chords, V, assign="lowest")
        z = ddsp.render_notes(lowest, T, ae.decoder.harmonics.sample_rate, hop, **options)
        torch.manual_seed(11)
        same = voices.mix_voices(ae.play(lowest, frames=T, **options), V, active=z["voiced"], hop_length=hop, hold=1, fade=2,
                                 pan=mix["pan"], gain=mix["gain"])
        assert gated.shape == (2, 2, T * hop) and torch.equal(gated, same)
