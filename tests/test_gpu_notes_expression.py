"""`note_expression` and `render_notes(..., expression=...)` on the device (csrc/ddsp_notes.hip: notes_expression_kernel and the
expressive instantiation of notes_render_kernel) against the plain loops of tests/notes_expression_reference.py, and
`AutoEncoder.transcribe(x, expression=True)` / `AutoEncoder.play(notes, expression=...)`.

Tolerances: as tests/test_notes_expression_host.py -- bend, owner, position and the fill values to the bit, normalized_cents to
the bit on the reference's position, f0 and loudness within 1 fp32 ulp (a NaN loudness a NaN), a position with synthetic vibrato
within 1 unit.  The 2051-row case is compared with the CPU path, which tests/test_notes_expression_host.py pins to the loops."""
import numpy as np
import pytest
import torch

import ddsp_pytorch_amd as ddsp
import notes_expression_reference as xref
import notes_reference as nref
import tuning_reference as ref
from ddsp_pytorch_amd.notes import extract_notes, note_expression, render_notes
from ddsp_pytorch_amd.tuning import TuningStatistics
from encoder_common import AEConf
from test_gpu_notes import tones
from test_notes_expression_host import (SHAPES_T, check_amounts, check_edits_carry_the_curve, check_expr_render, check_no_expression_is_no_change,
                                        check_round_trip, check_stretched_ramp, check_tile_boundaries, close_levels, crowded_case, expression_of,
                                        make_source, run_expr_case, run_expr_render_cases, run_expression_cases)
from test_notes_host import HOP, RECORDS, SR, check_records, make_records, notes_of, records_of
from test_tuning_host import same_bits, within_one_ulp, z_of

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("T", SHAPES_T)
def test_device_expression_equals_plain_loops(T):
    run_expression_cases(T, "cuda")


@pytest.mark.parametrize("T", SHAPES_T)
def test_device_expressive_render_equals_plain_loops(T):
    run_expr_render_cases(T, "cuda")


def test_no_expression_is_no_change_on_the_device():
    check_no_expression_is_no_change("cuda")


def test_round_trip_and_edits_on_the_device():
    check_round_trip("cuda")
    check_edits_carry_the_curve("cuda")


def test_stretch_and_amounts_on_the_device():
    check_stretched_ramp("cuda")
    check_amounts("cuda")


def test_tile_boundaries_and_a_crowded_row():
    check_tile_boundaries("cuda")
    rec, src, source = crowded_case()
    run_expr_case(rec, [5], 40, src, source, "cuda", dict(glide=4, keep_attack=1), "crowded")
    x = ref.make(743, 2, 40)
    e = note_expression(z_of(x, "cuda", keys=("cents", "f0")), notes_of(rec, [5], "cuda"), return_owner=True)
    want = xref.expression(x["cents"], rec, [5])
    assert same_bits(e.bend.cpu().numpy(), want["bend"]) and same_bits(e.owner.cpu().numpy(), want["owner"])


def test_more_rows_than_a_few_tiles():
    """2051 rows of 5 frames, a workgroup each, against the CPU path: the expression, then an edited render that reads it"""
    x = ref.make(760, 2051, 5, special=True)
    stats = TuningStatistics(offset=-7, root=0, scale="chromatic")
    outs = []
    for device in ("cuda", "cpu"):
        z = z_of(x, device, keys=("cents", "f0", "loud"))
        notes = extract_notes(z, stats.to(device))
        e = note_expression(z, notes, return_owner=True)
        edited = notes.transpose(-2)._with(frames=torch.where(notes._used(), notes.frames + 1, notes.frames))
        out = render_notes(edited, 6, SR, HOP, expression=e, keep_attack=1, attack=2, return_info=True)
        outs.append(dict({k: v.cpu().numpy().reshape(2051, 6) for k, v in out.items()}, bend=e.bend.cpu().numpy(), own=e.owner.cpu().numpy()))
    got, host = outs
    for k in ("bend", "own", "owner", "position", "normalized_cents", "harmonicity", "voiced"):
        assert same_bits(got[k], host[k]), k
    assert within_one_ulp(got["f0"], host["f0"]) and close_levels(got["loudness"], host["loudness"])
    assert (got["own"] >= 0).any() and (got["own"] < 0).any() and got["bend"].any()


# ------------------------------------------------------------------------------------------------------------------ robustness
PAD = 256


def guarded(n, dtype):
    """n elements between two zones of 0x7F bytes"""
    size = n * torch.empty((), dtype=dtype).element_size()
    whole = torch.full((size + 2 * PAD,), 0x7F, device="cuda", dtype=torch.uint8)
    return whole, whole[PAD:PAD + size].view(dtype)


def guards_intact(whole):
    return bool((whole[:PAD] == 0x7F).all()) and bool((whole[-PAD:] == 0x7F).all())


OUT_TYPES = [torch.float32] * 4 + [torch.uint8, torch.int64, torch.int32]
OUT_KEYS = ("f0", "cents", "loudness", "harmonicity", "voiced", "position", "owner")


def raw_expression(cents, notes, B, T, N, bend, owner):
    ptr = lambda x: x.data_ptr() if x.numel() else None           # noqa: E731
    return ddsp._lib.lib().ddsp_notes_expression(cents.data_ptr(), *(ptr(getattr(notes, k)) for k in RECORDS[:4]), notes.count.data_ptr(),
                                                 notes.offset.data_ptr(), bend.data_ptr(), owner.data_ptr(), B, T, N, notes.groups,
                                                 torch.cuda.current_stream().cuda_stream)


def raw_render_expr(notes, e, source, B, T, N, outs):
    ptr = lambda x: x.data_ptr() if x is not None and x.numel() else None           # noqa: E731
    return ddsp._lib.lib().ddsp_notes_render_expr(
        *(ptr(getattr(notes, k)) for k in RECORDS[:5]), notes.count.data_ptr(), notes.offset.data_ptr(), *(o.data_ptr() for o in outs), B, T, N,
        notes.groups, 1, 3 * 65536, 2, 2, 3, 1, 4, 25.0 * 65536.0, 0.14, -2.0, 0.5, ptr(source), ptr(e.onset), ptr(e.frames), ptr(e.level),
        e.count.data_ptr(), e.bend.data_ptr(), ptr(e.loudness), e.source_frames, e.max_notes, -0.75, 1.5, 2, 1,
        torch.cuda.current_stream().cuda_stream)


RAW = dict(keep_detune=True, transpose_units=3 * 65536, glide=2, attack=2, release=3, delay=1, ramp=4, depth_units=25.0 * 65536.0, omega=0.14,
           floor=-2.0, default_level=0.5, bend_amount=-0.75, dyn_amount=1.5, keep_attack=2, keep_release=1)


@pytest.mark.parametrize("N,Nsrc", [(40, 33), (0, 5), (7, 0), (300, 300)])
def test_robustness_guard_zones_and_repeatability(N, Nsrc):
    """Records that do not match the track, a source with indices below -1 and beyond Nsrc, source notes that run past Tsrc and
    begin before 0, NaN source levels, NaN and +-inf in the source's loudness, counts above N, below 0 and 0, N = 0 and Nsrc = 0:
    the reference's values, every guard zone intact, and a second run gives equal bits."""
    B, T, Tsrc = 5, 300, 257
    x = ref.make(770 + N, B, T, special=True)
    rec = make_records(771 + N, B, N, T)
    rec["count"][:] = [N + 5, 0, N, 1 << 30, -3]
    src = make_source(772 + Nsrc, B, Tsrc, Nsrc)
    src["count"][:] = [Nsrc, Nsrc + 9, 0, -1, Nsrc]
    source = np.random.default_rng(773).integers(-5, Nsrc + 5, (B, N)).astype(np.int32)
    offset = [7, -50, 50, 0, 12]
    if N == 40:
        # a NaN, +inf and -inf where they are read for certain: the first frames of a valid source note, which the first note of row
        # 0 that sounds for three frames takes as its source (keep_attack = 2: its first two frames read them one to one)
        plain = nref.render(rec, offset, T)["owner"][0]
        i0 = next(i for i in range(N) if (plain == i).sum() >= 3)
        j0 = next(j for j in range(Nsrc) if src["onset"][0, j] >= 0 and src["frames"][0, j] >= 3 and
                  src["onset"][0, j] + src["frames"][0, j] <= Tsrc and not np.isnan(src["level"][0, j]))
        source[0, i0] = j0
        src["loudness"][0, src["onset"][0, j0]:src["onset"][0, j0] + 3] = [np.nan, np.inf, -np.inf]
    notes, e = notes_of(rec, offset, "cuda"), expression_of(src, "cuda")
    cents = torch.from_numpy(x["cents"]).cuda()
    source_dev = torch.from_numpy(source).cuda()
    bend_w, bend = guarded(B * T, torch.int32)
    owner_w, owner = guarded(B * T, torch.int32)
    wholes = [guarded(B * T, dt) for dt in OUT_TYPES]
    want_e = xref.expression(x["cents"], rec, offset)
    want = xref.render_expr(rec, offset, T, src, source=source, **RAW)
    runs = []
    for _ in range(2):
        assert raw_expression(cents, notes, B, T, N, bend, owner) == 0
        assert raw_render_expr(notes, e, source_dev, B, T, N, [o for _, o in wholes]) == 0
        torch.cuda.synchronize()
        assert guards_intact(bend_w) and guards_intact(owner_w) and all(guards_intact(w) for w, _ in wholes)
        got = {k: o.view(B, T).cpu().numpy() for k, (_, o) in zip(OUT_KEYS, wholes)}
        got["voiced"] = got["voiced"].astype(bool)
        assert same_bits(bend.view(B, T).cpu().numpy(), want_e["bend"]) and same_bits(owner.view(B, T).cpu().numpy(), want_e["owner"])
        check_expr_render(got, want, ("guarded", N, Nsrc), vibrato=True)
        runs.append(dict(got, bend=bend.cpu().numpy().copy()))
    assert all(same_bits(runs[0][k], runs[1][k]) for k in runs[0])
    if N == 40:
        assert np.isnan(want["loudness"]).any() and np.isinf(want["loudness"]).any() and (want["owner"] >= 0).any() and want_e["bend"].any()


def test_both_calls_in_one_graph_replayed_on_changed_inputs():
    B, T, N = 3, 300, 65
    xs = [ref.make(780 + i, B, T, special=True) for i in range(3)]
    recs = [make_records(783 + i, B, N, T) for i in range(3)]
    buf = z_of(xs[0], "cuda", keys=("cents", "f0", "loud"))
    notes = notes_of(recs[0], [3], "cuda")
    options = dict(glide=3, release=4, keep_attack=1, keep_release=2, bend_amount=0.5, transpose=-1.25)

    def launch():
        e = note_expression(buf, notes, return_owner=True)
        longer = notes._with(frames=torch.where(notes._used(), notes.frames * 2, notes.frames))
        return e, render_notes(longer, T, SR, HOP, return_info=True, expression=e, **options)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            e, captured = launch()
    torch.cuda.current_stream().wait_stream(side)
    for x, rec in zip(xs[1:], recs[1:]):
        for k, v in z_of(x, "cpu", keys=("cents", "f0", "loud")).items():
            buf[k].copy_(v)
        for k in RECORDS:
            getattr(notes, k).copy_(torch.from_numpy(rec[k]))
        captured["position"].fill_(-9)
        e.bend.fill_(-9)
        graph.replay()
        torch.cuda.synchronize()
        want_e = xref.expression(x["cents"], rec, [3])
        assert same_bits(e.bend.cpu().numpy(), want_e["bend"]) and same_bits(e.owner.cpu().numpy(), want_e["owner"])
        n = np.minimum(np.maximum(rec["count"], 0), N)
        used = np.arange(N)[None] < n[:, None]
        longer = dict(rec, frames=np.where(used, rec["frames"] * 2, rec["frames"]).astype(np.int32))
        src = dict(onset=rec["onset"], frames=rec["frames"], level=rec["level"], count=rec["count"], bend=want_e["bend"], loudness=x["loud"])
        want = xref.render_expr(longer, [3], T, src, bend_amount=0.5, keep_attack=1, keep_release=2,
                                **{k: v for k, v in dict(glide=3, release=4, transpose_units=round(-1.25 * ref.S)).items()})
        got = {k: v.cpu().numpy().reshape(B, T) for k, v in captured.items()}
        got["cents"] = got.pop("normalized_cents")
        check_expr_render(got, want, "replay")
        assert (want["owner"] >= 0).any() and (want["position"] != nref.render(longer, [3], T, glide=3, release=4,
                                                                                  transpose_units=round(-1.25 * ref.S))["position"]).any()


# ------------------------------------------------------------------------------------------------------------------ end to end
def test_autoencoder_transcribe_and_play_with_expression():
    ae = ddsp.AutoEncoder(AEConf, tracker='yin').cuda().eval()
    x = tones().cuda()
    pad = (ae.padding // 2, ae.padding - ae.padding // 2)
    options = dict(tuning=TuningStatistics(offset=0, root=0, scale="chromatic").to("cuda"), min_note_frames=2, hysteresis=30.0)
    with torch.no_grad():
        z = ae.encoder(torch.nn.functional.pad(x, pad))
        T = z["f0"].shape[1]
        notes, e = ae.transcribe(x, expression=True, **options)
        check_records(records_of(notes), records_of(extract_notes(z, **options)), "transcribe")
        want = note_expression(z, notes)
        assert same_bits(e.bend.cpu().numpy(), want.bend.cpu().numpy()) and torch.equal(e.loudness, z["loudness"].reshape(2, T))
        assert int(notes.count.min()) >= 1 and e.source_frames == T
        hop, rate = ae.hop_length, ae.decoder.harmonics.sample_rate
        for played, render in ((notes, dict(floor=-4.0)),
                               (notes.transpose(2), dict(floor=-4.0, keep_attack=2, keep_release=2, bend_amount=0.5, dynamics_amount=0.8, release=2))):
            zr = render_notes(played, T, rate, hop, expression=e, **render)
            torch.manual_seed(11)
            expected = ae.decoder(zr)
            torch.manual_seed(11)
            audio = ae.play(played, frames=T, expression=e, **render)
            assert torch.equal(audio, expected) and audio.shape == (2, T * hop) and bool(torch.isfinite(audio).all())
        assert float(audio.abs().max()) > 0
