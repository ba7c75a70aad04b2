"""`extract_notes` and `render_notes` on the device (csrc/ddsp_notes.hip) against the plain-loop definition of
tests/notes_reference.py, and `AutoEncoder.transcribe` / `AutoEncoder.play`.

Tolerances: as tests/test_notes_host.py -- every integer output, the fill values, `level` and normalized_cents to the bit, f0
and loudness within 1 fp32 ulp, a position with vibrato within 1 unit.  The 2051-row case is compared with the CPU path, which
tests/test_notes_host.py pins to the plain loops, and a few of its rows with the loops themselves."""
import numpy as np
import pytest
import torch

import ddsp_pytorch_amd as ddsp
import notes_reference as nref
import tuning_reference as ref
from ddsp_pytorch_amd.conditioning import ConditioningStatistics, fit_conditioning
from ddsp_pytorch_amd.notes import Notes, extract_notes, render_notes
from ddsp_pytorch_amd.tuning import TuningStatistics
from encoder_common import AEConf
from test_notes_host import (EXTRACT_SHAPES, GATES, HOP, RECORDS, RENDER_OPTIONS, RENDER_T, SR, check_against_tune_pitch,
                             check_designed_extraction, check_designed_render, check_max_notes, check_melody, check_records, check_render,
                             check_round_trip, got_extract, got_render, hand_tuning, loop_options, make_records, notes_of, records_of,
                             run_extract_cases, run_render_cases, want_extract)
from test_tuning_host import same_bits, z_of

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("R,T", EXTRACT_SHAPES)
def test_device_extraction_equals_plain_loops(R, T):
    run_extract_cases(R, T, "cuda")


def test_extraction_properties_hold_on_the_device():
    check_designed_extraction("cuda")
    check_max_notes("cuda")
    check_against_tune_pitch("cuda")
    check_melody("cuda")


def test_a_long_row():
    x = ref.make(171, 1, 4099, special=True)
    for gate, options in ((GATES[0], dict()), (GATES[1], dict(min_note_frames=3, hysteresis=0.0))):
        stats, offset, root = hand_tuning(171, 1, gate, "cuda")
        want = want_extract(x, gate, offset, root, 0xAB5, 4099 // max(1, options.get("min_note_frames", 0)), **options)
        _, got = got_extract(x, "cuda", stats, gate, **options)
        check_records(got, want, ("4099 frames", options))
        assert want["count"][0] > 100


def test_more_rows_than_the_grid():
    """2051 rows of 5 frames, a workgroup each: more rows than the 2048 the tuning kernels keep in flight, every one checked."""
    gate = GATES[1]
    x = ref.make(172, 2051, 5, special=True)
    stats, offset, root = hand_tuning(172, 2051, gate, "cuda")
    _, got = got_extract(x, "cuda", stats, gate)
    _, host = got_extract(x, "cpu", stats.to("cpu"), gate)
    check_records(got, host, "2051 rows")
    rows = [0, 1, 2, 3, 2046, 2047, 2048, 2049, 2050]
    want = want_extract({k: v[rows] for k, v in x.items()}, gate, offset[rows], root[rows], 0xAB5, 5)
    check_records({k: v[rows] for k, v in got.items()}, want, "2051 rows, against the loops")
    assert got["count"].max() >= 2 and (got["count"] == 0).any()


GUARD = 51                                                      # fits every output type, the voiced bytes included


def guarded(n, dtype, pad=64):
    whole = torch.full((n + 2 * pad,), GUARD, device="cuda", dtype=dtype)
    return whole, whole[pad:pad + n]


def guards_intact(whole, n, pad=64):
    return bool((whole[:pad] == GUARD).all()) and bool((whole[pad + n:] == GUARD).all())


def raw_extract(z, stats, B, T, N, outs, count, min_note=3, hysteresis=20 * 65536):
    n, h, l = (z[k].contiguous() for k in ("normalized_cents", "harmonicity", "loudness"))
    v = z["voiced"].contiguous().view(torch.uint8)
    ptr = lambda x: x.data_ptr() if x.numel() else None           # noqa: E731
    return ddsp._lib.lib().ddsp_notes_extract(n.data_ptr(), h.data_ptr(), l.data_ptr(), v.data_ptr(), stats.offset.data_ptr(),
                                              stats.root.data_ptr(), *(ptr(o) for o in outs), count.data_ptr(), B, T, N, stats.groups, 0xAB5, -1,
                                              hysteresis, min_note, 1, -3.0, 0.2, torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("N", [172 // 3, 4, 1, 0])
def test_extraction_guard_zones_and_overflow(N):
    """guard zones around every output; with N below the count nothing is written past N, and count still counts every note"""
    B, T, gate = 5, 172, GATES[1]
    x = ref.make(176, B, T, special=True)
    stats, offset, root = hand_tuning(176, B, gate, "cuda")
    z = z_of(x, "cuda", True)
    wholes = [guarded(B * N, torch.float32 if k == "level" else torch.int32) for k in RECORDS[:5]]
    count_w, count = guarded(B, torch.int32)
    for _ in range(2):                                          # a second run gives equal bits
        assert raw_extract(z, stats, B, T, N, [o for _, o in wholes], count) == 0
        torch.cuda.synchronize()
        assert all(guards_intact(w, B * N) for w, _ in wholes) and guards_intact(count_w, B)
        want = want_extract(x, gate, offset, root, 0xAB5, N, min_note_frames=3)
        got = dict({k: o.view(B, N).cpu().numpy() for k, (_, o) in zip(RECORDS[:5], wholes)}, count=count.cpu().numpy())
        check_records(got, want, ("guarded", N))
    assert (want["count"] > N).any() if N <= 4 else (want["count"] <= N).all()


def test_extraction_graph_replay_on_changed_inputs_equals_eager():
    B, T = 3, 172
    first, later, last = ref.make(177, B, T), ref.make(178, B, T, special=True), ref.make(179, B, T)
    stats, _, _ = hand_tuning(177, B, GATES[1], "cuda")
    buf = z_of(first, "cuda", True)
    launch = lambda: extract_notes(buf, stats, min_note_frames=2, max_notes=40)        # noqa: E731
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()                                                # warm-up on the capture stream
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            captured = launch()
    torch.cuda.current_stream().wait_stream(side)
    for x in (later, last):
        for k, v in z_of(x, "cpu", True).items():
            buf[k].copy_(v)
        captured.count.fill_(-9)
        captured.pitch.fill_(-9)
        graph.replay()
        torch.cuda.synchronize()
        eager = extract_notes(z_of(x, "cuda", True), stats, min_note_frames=2, max_notes=40)
        check_records(records_of(captured), records_of(eager), "replay")
        assert int(eager.count.max()) > 3


# ------------------------------------------------------------------------------------------------------------------ the render
@pytest.mark.parametrize("T", RENDER_T)
def test_device_render_equals_plain_loops(T):
    run_render_cases(T, "cuda")


def test_render_of_designed_note_lists_and_round_trips():
    check_designed_render("cuda")
    check_round_trip("cuda")


def test_render_of_a_long_row():
    """T = 4097: seventeen tiles of 256 frames; 300 notes a row are staged tile by tile, 3000 crowd more than 320 records into a
    tile, which then reads them from global memory"""
    T = 4097
    for N, options in ((300, RENDER_OPTIONS[5]), (300, RENDER_OPTIONS[15]), (3000, RENDER_OPTIONS[11])):
        rec = make_records(300 + N, 2, N, T)
        rec["count"][:] = N
        want = nref.render(rec, [-9], T, **loop_options(options))
        got = got_render(notes_of(rec, [-9], "cuda"), T, **options)
        check_render(got, want, (T, N, options), vibrato="vibrato_cents" in options)
    # every note on the same few frames: one tile's candidates exceed the staging area at any T
    rec = make_records(301, 2, 400, 40)
    rec["count"][:] = 400
    want = nref.render(rec, [5], 40, **loop_options(RENDER_OPTIONS[2]))
    check_render(got_render(notes_of(rec, [5], "cuda"), 40, **RENDER_OPTIONS[2]), want, "crowded")


def raw_render(notes, B, T, N, outs, flags=1, glide=2, attack=2, release=3):
    ptr = lambda x: x.data_ptr() if x.numel() else None           # noqa: E731
    return ddsp._lib.lib().ddsp_notes_render(*(ptr(getattr(notes, k)) for k in RECORDS[:5]), notes.count.data_ptr(), notes.offset.data_ptr(),
                                             *(o.data_ptr() for o in outs), B, T, N, notes.groups, flags, 3 * 65536, glide, attack, release, 1, 4,
                                             25.0 * 65536.0, 0.14, -2.0, 0.5, torch.cuda.current_stream().cuda_stream)


RAW = dict(transpose=3.0 / 100.0, glide=2, attack=2, release=3, vibrato_cents=25.0, vibrato_delay=1, vibrato_ramp=4, floor=-2.0, default_level=0.5)
OUT_TYPES = [torch.float32] * 4 + [torch.uint8, torch.int64, torch.int32]


def raw_outputs(got_outs, B, T):
    keys = ("f0", "cents", "loudness", "harmonicity", "voiced", "position", "owner")
    got = {k: o.view(B, T).cpu().numpy() for k, o in zip(keys, got_outs)}
    got["voiced"] = got["voiced"].astype(bool)
    return got


@pytest.mark.parametrize("T,N", [(172, 65), (700, 300), (1, 0)])
def test_render_guard_zones_and_repeatability(T, N):
    B = 3
    rec = make_records(310 + T, B, N, T)
    notes = notes_of(rec, [7, -50, 50], "cuda")
    wholes = [guarded(B * T, dt) for dt in OUT_TYPES]
    options = loop_options(dict(RAW, vibrato_hz=0.0))
    options["omega"] = 0.14
    want = nref.render(rec, [7, -50, 50], T, **options)
    runs = []
    for _ in range(2):
        assert raw_render(notes, B, T, N, [o for _, o in wholes]) == 0
        torch.cuda.synchronize()
        assert all(guards_intact(w, B * T) for w, _ in wholes)
        runs.append(raw_outputs([o for _, o in wholes], B, T))
        check_render(runs[-1], want, ("guarded", T, N), vibrato=True)
    assert all(same_bits(runs[0][k], runs[1][k]) for k in runs[0])


def test_unsorted_onsets_stay_in_bounds():
    """onsets in no order: the values are unspecified; the call returns and every guard zone is intact"""
    B, T, N = 3, 300, 500
    rec = make_records(320, B, N, T)
    rng = np.random.default_rng(320)
    rec["onset"] = rng.integers(-(1 << 31), 1 << 31, (B, N)).astype(np.int32)
    rec["onset"][1] = rng.integers(-50, T + 50, N)
    rec["frames"][2] = rng.integers(-(1 << 31), 1 << 31, N)
    rec["count"][:] = [N, N + 5, 1 << 30]
    notes = notes_of(rec, [0], "cuda")
    wholes = [guarded(B * T, dt) for dt in OUT_TYPES]
    guard_in = [guarded(B * N, torch.float32 if k == "level" else torch.int32) for k in RECORDS[:5]]
    for (_, inner), k in zip(guard_in, RECORDS[:5]):             # the records between guard zones as well: reads past them would show as notes
        inner.copy_(getattr(notes, k).reshape(-1))
        setattr(notes, k, inner.view(B, N))
    for glide in (0, 5):
        assert raw_render(notes, B, T, N, [o for _, o in wholes], glide=glide) == 0
        torch.cuda.synchronize()
        assert all(guards_intact(w, B * T) for w, _ in wholes)
    owner = wholes[6][1].view(B, T).cpu().numpy()
    assert owner.min() >= -1 and owner.max() < N


def test_render_graph_replay_on_changed_inputs_equals_eager():
    B, T, N = 3, 172, 65
    recs = [make_records(330 + i, B, N, T) for i in range(3)]
    notes = notes_of(recs[0], [3], "cuda")
    options = dict(glide=3, attack=2, release=4, vibrato_cents=15.0, vibrato_delay=2, vibrato_ramp=4, transpose=-1.25)
    launch = lambda: render_notes(notes, T, SR, HOP, return_info=True, **options)      # noqa: E731
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            captured = launch()
    torch.cuda.current_stream().wait_stream(side)
    for rec in recs[1:]:
        for k in RECORDS:
            getattr(notes, k).copy_(torch.from_numpy(rec[k]))
        captured["position"].fill_(-9)
        captured["f0"].zero_()
        graph.replay()
        torch.cuda.synchronize()
        eager = render_notes(notes_of(rec, [3], "cuda"), T, SR, HOP, return_info=True, **options)
        for k in eager:
            assert same_bits(captured[k].cpu().numpy(), eager[k].cpu().numpy()), k
        assert int(eager["owner"].max()) > 10


# ------------------------------------------------------------------------------------------------------------------ entry points
def test_argument_checks_return_before_any_launch():
    B, T, N = 2, 20, 6
    x = ref.make(340, B, T)
    z = z_of(x, "cuda", True)
    stats, _, _ = hand_tuning(340, B, {}, "cuda")
    outs = [torch.full((B * N,), GUARD, device="cuda", dtype=torch.float32 if k == "level" else torch.int32) for k in RECORDS[:5]]
    count = torch.full((B,), GUARD, device="cuda", dtype=torch.int32)
    assert raw_extract(z, stats, B, T, N, outs, count, min_note=-1) == -1 and raw_extract(z, stats, B, T, N, outs, count, hysteresis=1201 * 65536) == -1
    assert raw_extract(z, stats, B, 1 << 24, N, outs, count) == -2 and raw_extract(z, stats, B, T, 1 << 30, outs, count) == -2
    assert raw_extract(z, stats, 3, T, N, outs, count) == -1      # two groups, three rows
    notes = notes_of(make_records(341, B, N, T), [0], "cuda")
    routs = [torch.full((B * T,), GUARD, device="cuda", dtype=dt) for dt in OUT_TYPES]
    assert raw_render(notes, B, T, N, routs, flags=4) == -1 and raw_render(notes, B, T, N, routs, glide=-1) == -1
    assert raw_render(notes, B, T, N, routs, attack=1 << 24) == -1 and raw_render(notes, B, 1 << 24, N, routs) == -2
    assert raw_render(notes, B, T, 1 << 30, routs) == -2
    torch.cuda.synchronize()
    assert all(bool((o == GUARD).all()) for o in outs + [count] + routs)
    assert raw_extract(z, stats, B, T, N, outs, count) == 0 and raw_render(notes, B, T, N, routs) == 0      # and the good calls do write
    torch.cuda.synchronize()
    assert all(bool((o != GUARD).any()) for o in outs + [count] + routs)


def tones():
    """2 x 16384 samples at 44.1 kHz: each row two tones in turn, a few cents off the grid"""
    t = np.arange(8192) / 44100.0
    rows = [[220.0 * 2 ** (-0.30 / 12), 246.94], [330.0 * 2 ** (0.2 / 12), 293.66]]
    x = np.stack([np.concatenate([0.3 * np.sin(2 * np.pi * f * t) for f in row]) for row in rows])
    return torch.from_numpy((x + 1e-4 * np.random.default_rng(0).standard_normal(x.shape)).astype(np.float32))


def test_autoencoder_transcribe_and_play():
    ae = ddsp.AutoEncoder(AEConf, tracker='yin').cuda().eval()
    x = tones().cuda()
    pad = (ae.padding // 2, ae.padding - ae.padding // 2)
    options = dict(tuning=TuningStatistics(offset=0, root=0, scale="chromatic").to("cuda"), min_note_frames=2, hysteresis=30.0)
    with torch.no_grad():
        z = ae.encoder(torch.nn.functional.pad(x, pad))
        want = extract_notes(z, **options)
        notes = ae.transcribe(x, **options)
        check_records(records_of(notes), records_of(want), "transcribe")
        assert int(notes.count.min()) >= 1 and notes.source_frames == z["f0"].shape[1]
        own = ae.transcribe(x)                                  # tuning=None: every clip measured by itself
        check_records(records_of(own), records_of(extract_notes(z)), "transcribe, measured")

        score = Notes(onset=[[0, 12, 20], [2, 10, 30]], frames=[[12, 8, 10], [8, 20, 6]], pitch=[[57, 60, 64], [69, 67, 65]],
                      level=[[-1.0, -0.5, -1.5], [-2.0, -1.0, -1.0]]).to("cuda")
        render = dict(glide=2, attack=1, release=3, floor=-4.0, vibrato_cents=20.0, vibrato_delay=3, vibrato_ramp=4)
        hop, rate = ae.hop_length, ae.decoder.harmonics.sample_rate
        target = ConditioningStatistics(torch.linspace(-2.0, 1.0, 65)[None], torch.tensor([0.55])).to("cuda")
        for frames, tgt in ((40, None), (40, target), (None, None)):
            T = 36 if frames is None else frames               # frames=None: the end of the last note
            zr = render_notes(score, T, rate, hop, **render)
            if tgt is not None:
                zr = fit_conditioning(zr, tgt)
            torch.manual_seed(11)
            expected = ae.decoder(zr)
            torch.manual_seed(11)
            audio = ae.play(score, frames=frames, target=tgt, **render)
            assert torch.equal(audio, expected) and audio.shape == (2, T * hop) and bool(torch.isfinite(audio).all())
        assert float(audio.abs().max()) > 0
        with pytest.raises(ValueError):
            ae.play(score, frames=40, return_info=True)
