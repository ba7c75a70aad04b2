"""`tuning_statistics` and `tune_pitch` on the device (csrc/ddsp_tuning.hip) against the plain-loop definition of
tests/tuning_reference.py, and `AutoEncoder.transfer(..., tune=...)`.

Tolerances: as tests/test_tuning_host.py -- histogram, offset, root, profile, notes, correction and normalized_cents to the
bit, f0 within 1 fp32 ulp (it is formed through exp2).  The largest pooled case is compared with the CPU path, which
tests/test_tuning_host.py pins to the plain loops; looping over half a million frames in Python would take minutes."""
import numpy as np
import pytest
import torch

import ddsp_pytorch_amd as ddsp
import tuning_reference as ref
from ddsp_pytorch_amd.conditioning import ConditioningStatistics, fit_conditioning
from ddsp_pytorch_amd.tuning import LDS_FRAMES, TuningStatistics, tune_pitch, tuning_statistics
from encoder_common import AEConf
from test_tuning_host import (GATES, OPTIONS, SHAPES, check_designed_ties, check_hard_snap_and_second_pass, check_identity_and_concert,
                              check_measures_itself, check_melody, check_stats, check_tune, check_vibrato_kept, got_stats, got_tune,
                              on_of, reference_options, run_cases, same_bits, z_of)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("R,T", SHAPES)
def test_device_equals_plain_loops(R, T):
    run_cases(R, T, "cuda")


def test_properties_hold_on_the_device():
    check_measures_itself("cuda")
    check_designed_ties("cuda")
    check_hard_snap_and_second_pass("cuda")
    check_vibrato_kept("cuda")
    check_identity_and_concert("cuda")
    check_melody("cuda")


def against_loops(x, gate, options_list, where, per_row=True, scale="major"):
    on = on_of(x, gate)
    want = ref.statistics(x["cents"], on, per_row=per_row, mask=ref.SCALES[scale])
    stats, got = got_stats(x, "cuda", gate, per_row=per_row, scale=scale)
    check_stats(got, want, where)
    results = []
    for options in options_list:
        call, loops = reference_options(options, x["cents"].shape[0], 7)
        exp = ref.tune(x["cents"], x["f0"], on, want["offset"], want["root"], ref.SCALES[scale], **loops)
        check_tune(got_tune(x, "cuda", stats, gate, **call), exp, (where, options))
        results.append(exp)
    return results


def test_rows_beyond_lds_take_the_workspace():
    T = LDS_FRAMES + 1
    assert ddsp._lib.lib().ddsp_tuning_workspace_bytes(2, T - 1) == 0 < ddsp._lib.lib().ddsp_tuning_workspace_bytes(2, T)
    for seed, n in ((71, T - 1), (72, T)):                      # the last row in LDS, the first in the workspace
        x = ref.make(seed, 2, n, special=True)
        against_loops(x, GATES[1], [OPTIONS[0], OPTIONS[6], OPTIONS[10], OPTIONS[12]], ("lds limit", n))


def designed_rows():
    """Two rows of 130 frames whose notes change where the kernel's tiles of 64 frames meet: a change in lane 63 and one in
    lane 0, notes that straddle a boundary, a run that ends on the last frame."""
    plans = [[(0, 63, 60), (63, 64, 62), (64, 101, 64), (121, 130, 65)],          # frames 101 .. 120 stay off
             [(0, 41, 60), (41, 91, 62), (91, 128, 64), (128, 130, 65)]]
    rng = np.random.default_rng(73)
    cents = np.full((2, 130), np.nan, dtype=np.float32)
    notes = np.full((2, 130), ref.OFF, dtype=np.int64)
    for b, plan in enumerate(plans):
        for first, last, note in plan:
            t = np.arange(first, last)
            c = 100.0 * note + 12.0 + 9.0 * np.sin(0.8 * t) + 2.0 * rng.standard_normal(last - first)
            cents[b, first:last] = ((c - ref.K) / 7180.0).astype(np.float32)
            notes[b, first:last] = note
    f0 = ref.f0_of_cents(np.nan_to_num(cents, nan=0.5))
    return dict(cents=cents, f0=f0, harm=np.ones_like(cents), loud=np.zeros_like(cents), voiced=np.ones(cents.shape, dtype=bool)), notes


def test_notes_at_the_tile_boundaries():
    x, notes = designed_rows()
    results = against_loops(x, {}, [dict(), dict(vibrato=False), dict(glide=4, min_note_frames=2), dict(glide=200, concert=True),
                                    dict(hysteresis=0.0, min_note_frames=3)], "tile boundaries")
    assert np.array_equal(results[0]["notes"], notes)           # the loops see the notes as planned: changes at 63, 64 and 128
    assert notes[0, 62] != notes[0, 63] != notes[0, 64] and notes[1, 63] == notes[1, 64] and notes[1, 127] != notes[1, 128]
    assert notes[0, 129] != ref.OFF and notes[0, 110] == ref.OFF


def test_more_rows_than_any_grid():
    """2051 rows of 5 frames: three more than the statistics' and the estimate's grids.  Every row against the CPU path (which
    tests/test_tuning_host.py pins to the plain loops), the rows either side of the grid's end against the loops themselves:
    2051 estimates in plain Python take several seconds."""
    gate = GATES[1]
    x = ref.make(74, 2051, 5, special=True)
    on = on_of(x, gate)
    stats, got = got_stats(x, "cuda", gate, per_row=True)
    check_stats(got, got_stats(x, "cpu", gate, per_row=True)[1], "2051 rows")
    rows = [0, 1, 2, 2046, 2047, 2048, 2049, 2050]
    want = ref.statistics(x["cents"][rows], [on[r] for r in rows], per_row=True)
    check_stats({k: v[rows] for k, v in got.items()}, want, "2051 rows, against the loops")
    for options in (dict(), dict(vibrato=False, glide=1)):
        out = got_tune(x, "cuda", stats, gate, **options)
        check_tune(out, got_tune(x, "cpu", stats.to("cpu"), gate, **options), ("2051 rows", options))
        exp = ref.tune(x["cents"][rows], x["f0"][rows], [on[r] for r in rows], want["offset"], want["root"], 0xAB5, h=20 * 65536, **options)
        check_tune({k: v[rows] for k, v in out.items()}, exp, ("2051 rows, against the loops", options))
    assert int(np.abs(out["correction"]).max()) > 0
    _, got = got_stats(x, "cuda", gate, per_row=False)
    check_stats(got, ref.statistics(x["cents"], on, per_row=False), "2051 rows pooled")


@pytest.mark.parametrize("R,T,loops", [(300, 7, True), (1, 20000, True), (3, 174789, False)])
def test_pooled_merge_is_exact_and_order_free(R, T, loops):
    """several workgroups add into one histogram; at 524 367 frames every workgroup walks more than one unit"""
    x = ref.make(75, R, T, special=True)
    gate = GATES[1]
    stats, got = got_stats(x, "cuda", gate)
    if loops:
        check_stats(got, ref.statistics(x["cents"], on_of(x, gate)), (R, T))
    else:
        assert R * T == 524367 > 512 * 1024
        check_stats(got, got_stats(x, "cpu", gate)[1], (R, T))
    assert got["frames"][0] > 100 and (got["histogram"][0] > 0).sum() > 50
    check_stats(got_stats(x, "cuda", gate)[1], got, "a second run")
    perm = np.random.default_rng(3).permutation(R)
    check_stats(got_stats({k: v[perm] for k, v in x.items()}, "cuda", gate)[1], got, "rows permuted")
    if R == 1:                                                  # one row: permute its frames instead
        perm = np.random.default_rng(4).permutation(T)
        check_stats(got_stats({k: v[:, perm] for k, v in x.items()}, "cuda", gate)[1], got, "frames permuted")


def guarded(n, dtype, pad=64):
    whole = torch.full((n + 2 * pad,), -77, device="cuda", dtype=dtype)
    return whole, whole[pad:pad + n]


def guards_intact(whole, n, pad=64):
    return bool((whole[:pad] == -77).all()) and bool((whole[pad + n:] == -77).all())


@pytest.mark.parametrize("pooled,T", [(False, 172), (True, 172), (False, LDS_FRAMES + 1)])
def test_guard_zones_stay_untouched(pooled, T):
    L = ddsp._lib.lib()
    R = 5
    x = ref.make(76, R, T, special=True)
    z = z_of(x, "cuda", True)
    n, f, h, l = (z[k].contiguous() for k in ("normalized_cents", "f0", "harmonicity", "loudness"))
    v = z["voiced"].contiguous().view(torch.uint8)
    G = 1 if pooled else R
    words = L.ddsp_tuning_accum_bytes(G) // 4
    accum_w, accum = guarded(words, torch.int32)
    off_w, off = guarded(G, torch.int32)
    root_w, root = guarded(G, torch.int32)
    prof_w, prof = guarded(G * 12, torch.int64)
    fr_w, fr = guarded(G, torch.int64)
    stream = torch.cuda.current_stream().cuda_stream
    assert L.ddsp_tuning_stats(n.data_ptr(), h.data_ptr(), l.data_ptr(), v.data_ptr(), accum.data_ptr(), R, T, int(pooled), -3.0, 0.2,
                               stream) == 0
    assert L.ddsp_tuning_estimate(accum.data_ptr(), off.data_ptr(), root.data_ptr(), prof.data_ptr(), fr.data_ptr(), G, 0xAB5, -1,
                                  stream) == 0
    outs = [guarded(R * T, torch.float32) for _ in range(2)] + [guarded(R * T, torch.int32) for _ in range(2)]
    nbytes = L.ddsp_tuning_workspace_bytes(R, T)
    assert (nbytes > 0) == (T > LDS_FRAMES)
    work_w, work = guarded(max(nbytes // 8, 1), torch.int64)
    assert L.ddsp_tuning_apply(f.data_ptr(), n.data_ptr(), h.data_ptr(), l.data_ptr(), v.data_ptr(), off.data_ptr(), root.data_ptr(), None,
                               outs[0][1].data_ptr(), outs[1][1].data_ptr(), outs[2][1].data_ptr(), outs[3][1].data_ptr(),
                               work.data_ptr() if nbytes else None, R, T, G, 0xAB5, -1, 20 * 65536, 3, 2, 1, 1.0, -3.0, 0.2, stream) == 0
    torch.cuda.synchronize()
    for whole, count in ((accum_w, words), (off_w, G), (root_w, G), (prof_w, G * 12), (fr_w, G), (work_w, max(nbytes // 8, 1))):
        assert guards_intact(whole, count)
    assert all(guards_intact(w, R * T) for w, _ in outs)
    on = on_of(x, GATES[1])
    want = ref.statistics(x["cents"], on, per_row=not pooled)
    assert same_bits(off.cpu().numpy(), want["offset"]) and same_bits(root.cpu().numpy(), want["root"])
    assert same_bits(prof.view(G, 12).cpu().numpy(), want["profile"]) and same_bits(fr.cpu().numpy(), want["frames"])
    exp = ref.tune(x["cents"], x["f0"], on, want["offset"], want["root"], 0xAB5, h=20 * 65536, min_note_frames=3, glide=2)
    got = dict(f0=outs[0][1].view(R, T).cpu().numpy(), cents=outs[1][1].view(R, T).cpu().numpy(),
               notes=outs[2][1].view(R, T).cpu().numpy(), correction=outs[3][1].view(R, T).cpu().numpy())
    check_tune(got, exp, ("guarded", pooled, T))


def test_graph_replay_on_changed_inputs_equals_eager():
    B, T = 3, 172
    first, later, last = ref.make(77, B, T), ref.make(78, B, T, special=True), ref.make(79, B, T)
    tuning = tuning_statistics(z_of(ref.make(80, B, 300), "cuda"), per_row=True)       # measured once, on other frames
    buf = z_of(first, "cuda", True)
    rows = torch.tensor([1.0, 0.5, 0.25], device="cuda")

    def launch():
        return tune_pitch(buf, tuning, amount=rows, glide=2, min_note_frames=2, return_info=True)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()                                                # warm-up on the capture stream
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            captured, info = launch()
    torch.cuda.current_stream().wait_stream(side)
    for x in (later, last):
        for k, v in z_of(x, "cpu", True).items():
            buf[k].copy_(v)
        for k in ("f0", "normalized_cents"):
            captured[k].zero_()
        info["notes"].fill_(-9)
        graph.replay()
        torch.cuda.synchronize()
        eager, eager_info = tune_pitch(z_of(x, "cuda", True), tuning, amount=rows, glide=2, min_note_frames=2, return_info=True)
        for k in ("f0", "normalized_cents"):
            assert same_bits(captured[k].cpu().numpy(), eager[k].cpu().numpy()), k
        assert torch.equal(info["notes"], eager_info["notes"]) and torch.equal(info["correction"], eager_info["correction"])
        assert int(eager_info["correction"].abs().max()) > 0


def tones(seed=0):
    """2 x 8192 samples at 44.1 kHz: two tones, 30 and 20 cents off the grid, both swelling"""
    t = np.arange(8192) / 44100.0
    swell = 0.2 + 0.8 * np.linspace(0, 1, 8192) ** 2
    x = np.stack([0.2 * swell * np.sin(2 * np.pi * 220.0 * 2 ** (-0.30 / 12) * t), 0.4 * swell * np.sin(2 * np.pi * 330.0 * 2 ** (0.2 / 12) * t)])
    return torch.from_numpy((x + 1e-4 * np.random.default_rng(seed).standard_normal(x.shape)).astype(np.float32))


def test_autoencoder_transfer_tunes_after_fitting():
    ae = ddsp.AutoEncoder(AEConf, tracker='yin').cuda().eval()
    x = tones().cuda()
    pad = (ae.padding // 2, ae.padding - ae.padding // 2)
    target = ConditioningStatistics(torch.linspace(-2.0, 1.0, 65)[None], torch.tensor([0.55])).to("cuda")
    options = dict(tuning=TuningStatistics(offset=0, root=0, scale="chromatic").to("cuda"), vibrato=False, hysteresis=0.0)
    with torch.no_grad():
        fitted = fit_conditioning(ae.encoder(torch.nn.functional.pad(x, pad)), target, min_frames=4)
        for tune in (True, options):
            tuned, info = tune_pitch(fitted, return_info=True, **(tune if isinstance(tune, dict) else {}))
            torch.manual_seed(11)
            want = ae.decoder(tuned)
            torch.manual_seed(11)
            got = ae.transfer(x, target, min_frames=4, tune=tune)
            assert torch.equal(got, want)
        torch.manual_seed(11)
        untuned = ae.transfer(x, target, min_frames=4)
        torch.manual_seed(11)
        assert torch.equal(untuned, ae.transfer(x, target, min_frames=4, tune=None))
        torch.manual_seed(11)
        assert torch.equal(untuned, ae.decoder(fitted))
    assert int(info["correction"].abs().max()) > 0 and not torch.equal(got, untuned) and got.shape == untuned.shape
    assert not same_bits(tuned["f0"].cpu().numpy(), fitted["f0"].cpu().numpy())
    with pytest.raises(ValueError):
        ae.transfer(x, target, tune=dict(return_info=True))
