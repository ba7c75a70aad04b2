"""`extract_notes`, `render_notes`, the `Notes` edits and the MIDI files on CPU tensors (the numpy path of
ddsp_pytorch_amd/notes.py) against the plain-loop definition of tests/notes_reference.py, the properties that follow from the
definition, and the ABI's additions.  The helpers take a device, and tests/test_gpu_notes.py runs them on the kernels.

Tolerances, all derived.  Every integer output (onset, frames, pitch, detune, count, owner, position without vibrato) and the
fill values are held to the bit; so is `level`, a maximum of inputs.  normalized_cents is held to the bit against the
definition: p / 65536 is exact, the subtraction and the division are single correctly rounded fp64 operations that cannot be
contracted, then one rounding to fp32 -- on the reference's position, or with vibrato on the result's own position (two fp64
sines differ far below half a unit, so the positions then agree within 1 unit: a rounding tie of llrint).  f0 (through exp2) and
loudness (whose fp64 product may be contracted before the one fp32 rounding) are held within 1 fp32 ulp, the precedent of the
voicing and tuning tests.

The round-trip bound (DESIGN.md section 10e's hard-snap bound): a rendered note without glide or vibrato lies at an exact
integer position b, and its normalized_cents is n' = fl32((b / 65536 - K) / 7180); read back, its position carries half a unit
of llrint and 65536 * 7180 * ulp(n') / 2 units of that fp32 rounding, so the note's mean comes back within
65536 * 7180 * ulp(n') / 2 + 1 units of b."""
import ctypes
import math
import os
import struct
from fractions import Fraction

import numpy as np
import pytest
import torch

import ddsp_pytorch_amd as ddsp
import notes_reference as nref
import tuning_reference as ref
from ddsp_pytorch_amd.notes import Notes, extract_notes, render_notes
from ddsp_pytorch_amd.tuning import TuningStatistics, tune_pitch, tuning_statistics
from test_host_abi import declared_prototypes
from test_tuning_host import on_of, same_bits, within_one_ulp, z_of

NEW_SYMBOLS = ("ddsp_notes_extract", "ddsp_notes_render")
EXTRACT_SHAPES = [(1, 1), (1, 2), (3, 5), (2, 63), (2, 64), (2, 65), (2, 128), (2, 129), (5, 172)]
GATES = [dict(), dict(voiced=True, silence=-3.0, confidence=0.2), dict(silence=-3.0), dict(voiced=True), dict(confidence=0.2)]
RECORDS = ("onset", "frames", "pitch", "detune", "level", "count")
SR, HOP = 16000, 64
RENDER_T = [1, 63, 64, 65, 172]
RENDER_N = [0, 1, 64, 65, 300]
# every option on and off: glide 0, 1, 4 and longer than any note; attack and release 0, 1, 5 and longer than any note; detune,
# concert, a fractional transpose; vibrato off, and on with delay 0 and 3 and ramp 1 and 8
RENDER_OPTIONS = [dict(), dict(glide=1), dict(glide=4), dict(glide=1000), dict(attack=1), dict(attack=5, release=5),
                  dict(attack=1000, release=1000), dict(release=1), dict(detune=False), dict(concert=True), dict(transpose=2.37),
                  dict(transpose=-0.5, glide=4, detune=False, concert=True), dict(floor=-3.0, default_level=0.25, attack=5),
                  dict(vibrato_cents=35.0), dict(vibrato_cents=35.0, vibrato_delay=3, vibrato_ramp=8),
                  dict(vibrato_cents=20.0, vibrato_delay=0, vibrato_ramp=8, glide=4),
                  dict(vibrato_cents=20.0, vibrato_delay=3, vibrato_ramp=1, release=5, vibrato_hz=7.0)]


# ------------------------------------------------------------------------------------------------------------------ extraction
def hand_tuning(seed, groups, gate, device, scale="major"):
    """a tuning set by hand: the extraction is defined for any offset and root"""
    rng = np.random.default_rng(seed)
    offset, root = rng.integers(-50, 50, groups), rng.integers(0, 12, groups)
    stats = TuningStatistics(offset.tolist(), root.tolist(), scale=scale, silence=gate.get("silence"), confidence=gate.get("confidence", 0.0))
    return stats.to(device), offset, root


def records_of(notes):
    return {k: getattr(notes, k).cpu().numpy() for k in RECORDS}


def got_extract(x, device, stats, gate, keys=("cents", "f0", "harm", "loud"), **options):
    notes = extract_notes(z_of(x, device, gate.get("voiced", False), keys), stats, **options)
    assert notes.device.type == device and notes.source_frames == x["cents"].shape[1]
    return notes, records_of(notes)


def want_extract(x, gate, offset, root, mask, N, hysteresis=20.0, min_note_frames=0, loud=True):
    return nref.extract(x["cents"], on_of(x, gate), offset, root, mask, N, h=round(hysteresis * 65536.0), min_note_frames=min_note_frames,
                        loud=x["loud"] if loud else None)


def check_records(got, want, where):
    for k in RECORDS:
        assert same_bits(got[k], want[k]), (where, k, got[k], want[k])


def run_extract_cases(R, T, device):
    for seed, low in ((140 + R, False), (150 + T, True)):
        x = ref.make(seed, R, T, special=True, low=low)
        for g, gate in enumerate(GATES):
            for groups in sorted({1, R}):
                stats, offset, root = hand_tuning(seed + g, groups, gate, device)
                for options in (dict(), dict(hysteresis=0.0), dict(min_note_frames=3), dict(min_note_frames=3, hysteresis=0.0)):
                    N = T // max(1, options.get("min_note_frames", 0))
                    want = want_extract(x, gate, offset, root, 0xAB5, N, **options)
                    _, got = got_extract(x, device, stats, gate, **options)
                    check_records(got, want, (R, T, low, gate, groups, options))
    # a dict without loudness: every level is NaN; another scale and a forced root
    stats, offset, root = hand_tuning(7, R, {}, device, "pentatonic")
    want = want_extract(x, {}, offset, [5] * R, 0x5AD, T, loud=False)
    notes, got = got_extract(x, device, stats, {}, keys=("cents", "harm"), scale="minor", root=5)
    check_records(got, want, (R, T, "no loudness"))
    assert np.isnan(got["level"]).all() and notes.scale == "minor" and notes.root.tolist() == [5] * R and notes.mask == 0x5AD


@pytest.mark.parametrize("R,T", EXTRACT_SHAPES)
def test_cpu_extraction_equals_plain_loops(R, T):
    run_extract_cases(R, T, "cpu")


def designed_rows(T, plans):
    """rows whose notes lie as planned: (first, last, note) runs, every other frame off"""
    rng = np.random.default_rng(173)
    cents = np.full((len(plans), T), np.nan, dtype=np.float32)
    for b, plan in enumerate(plans):
        for first, last, note in plan:
            t = np.arange(first, last)
            c = 100.0 * note + 12.0 + 9.0 * np.sin(0.8 * t) + 2.0 * rng.standard_normal(last - first)
            cents[b, first:last] = ((c - ref.K) / 7180.0).astype(np.float32)
    loud = rng.standard_normal(cents.shape).astype(np.float32)
    return dict(cents=cents, f0=ref.f0_of_cents(np.nan_to_num(cents, nan=0.5)), harm=np.ones_like(cents), loud=loud,
                voiced=np.ones(cents.shape, dtype=bool))


# the kernel's tiles are 64 frames: a change in lane 63 and one in lane 0, notes that straddle one and two tile boundaries, a note
# that ends with a tile (the next tile emits it), a run that ends on the last frame, a row that is one note; with T = 192 the
# last frame is also a tile's last (the row's end emits the note)
DESIGNED = [(200, [[(0, 63, 60), (63, 64, 62), (64, 101, 64), (121, 200, 65)],
                   [(0, 41, 60), (41, 91, 62), (91, 128, 64), (128, 130, 65), (130, 192, 67)],
                   [(0, 200, 60)]]),
            (192, [[(0, 192, 60)], [(10, 64, 60), (64, 128, 62), (128, 192, 64)], [(0, 1, 60), (191, 192, 72)]])]


def check_designed_extraction(device):
    for T, plans in DESIGNED:
        x = designed_rows(T, plans)
        stats = TuningStatistics(offset=12, root=0, scale="chromatic").to(device)
        for options in (dict(), dict(min_note_frames=3), dict(hysteresis=0.0, min_note_frames=2)):
            N = T // max(1, options.get("min_note_frames", 0))
            want = want_extract(x, {}, 12, 0, 0xFFF, N, **options)
            _, got = got_extract(x, device, stats, {}, **options)
            check_records(got, want, (T, options))
            if "hysteresis" not in options:                      # the loops see the notes as planned
                for b, plan in enumerate(plans):
                    kept = [(f, l - f, n) for f, l, n in plan if l - f >= options.get("min_note_frames", 0)]
                    assert [tuple(int(want[k][b, i]) for k in ("onset", "frames", "pitch")) for i in range(want["count"][b])] == kept


def test_designed_rows_at_the_tile_boundaries():
    check_designed_extraction("cpu")


def check_max_notes(device):
    """N smaller than the count: count is the reference's and the first N records are; N = 1 and N = 0"""
    x = ref.make(161, 3, 172, special=True)
    stats, offset, root = hand_tuning(161, 3, {}, device)
    full = want_extract(x, {}, offset, root, 0xAB5, 172)
    assert full["count"].max() > 9
    for N in (7, 1, 0):
        want = want_extract(x, {}, offset, root, 0xAB5, N)
        notes, got = got_extract(x, device, stats, {}, max_notes=N)
        check_records(got, want, ("max_notes", N))
        assert same_bits(got["count"], full["count"]) and got["onset"].shape == (3, N)
        assert same_bits(got["pitch"], full["pitch"][:, :N]) and same_bits(got["detune"], full["detune"][:, :N])
        with pytest.raises(ValueError):
            notes.validate()
    extract_notes(z_of(x, device), stats).validate()


def test_max_notes_smaller_than_the_count():
    check_max_notes("cpu")


def check_against_tune_pitch(device):
    """the records, expanded to frames, are tune_pitch's notes; detune is minus its vibrato-kept correction"""
    x = ref.make(162, 4, 172, special=True)
    for gate in GATES[:2]:
        for groups in (1, 4):
            stats, _, _ = hand_tuning(162, groups, gate, device)
            z = z_of(x, device, gate.get("voiced", False))
            _, info = tune_pitch(z, stats, vibrato=True, amount=1.0, glide=0, concert=False, return_info=True)
            notes = extract_notes(z, stats, min_note_frames=0)
            frame_notes, frame_detune = nref.expand(records_of(notes), 172)
            assert same_bits(frame_notes, info["notes"].cpu().numpy())
            on = frame_notes != ref.OFF
            assert on.any() and np.array_equal(frame_detune[on], -info["correction"].cpu().numpy().astype(np.int64)[on])


def test_extraction_agrees_with_tune_pitch():
    check_against_tune_pitch("cpu")


# ------------------------------------------------------------------------------------------------------------------ the render
def make_records(seed, B, N, T):
    """Seeded note lists [B, N] with onsets in order (some before frame 0, some past T, many equal or touching), NaN levels and
    invalid records in the middle; the rows' counts cycle through 0, N and N + 5."""
    rng = np.random.default_rng(seed)
    rec = dict(onset=np.sort(rng.integers(-6, T + 6, (B, N)), axis=1).astype(np.int32), frames=rng.integers(1, 14, (B, N)).astype(np.int32),
               pitch=rng.integers(36, 96, (B, N)).astype(np.int32), detune=rng.integers(-40 * 65536, 40 * 65536, (B, N)).astype(np.int32),
               level=(rng.random((B, N)) * 2.0 - 1.0).astype(np.float32))
    rec["level"][rng.random((B, N)) < 0.15] = np.nan
    for k, value in (("frames", 0), ("pitch", nref.NO_PITCH), ("pitch", 128), ("pitch", -1), ("detune", (1 << 30) + 1), ("frames", -3)):
        if N > 8:
            rec[k][rng.integers(0, B), rng.integers(1, N - 1)] = value
    rec["count"] = np.array([(0, N, N + 5)[(b + seed) % 3] for b in range(B)], dtype=np.int32)
    return rec


def notes_of(rec, offset, device, **kw):
    kw.setdefault("root", [0] * len(offset))
    return Notes(*(torch.from_numpy(rec[k]) for k in RECORDS), offset=offset, **kw).to(device)


def loop_options(options):
    """render_notes' options -> the plain loops'"""
    o = dict(options)
    hz = o.pop("vibrato_hz", 5.5)
    return dict(keep_detune=o.pop("detune", True), concert=o.pop("concert", False), transpose_units=round(o.pop("transpose", 0.0) * ref.S),
                depth_units=o.pop("vibrato_cents", 0.0) * 65536.0, omega=2.0 * math.pi * (hz * HOP / SR), delay=o.pop("vibrato_delay", 0),
                ramp=o.pop("vibrato_ramp", 1), **o)


def got_render(notes, T, **options):
    z = render_notes(notes, T, SR, HOP, return_info=True, **options)
    B = notes.rows
    for k in ("f0", "normalized_cents", "loudness", "harmonicity", "voiced"):
        assert z[k].shape == (B, T, 1) and z[k].dtype == (torch.bool if k == "voiced" else torch.float32), k
    assert set(render_notes(notes, T, SR, HOP, **options)) == {"f0", "normalized_cents", "loudness", "harmonicity", "voiced"}
    out = {k: v.cpu().numpy().reshape(B, T) for k, v in z.items()}
    out["cents"] = out.pop("normalized_cents")
    return out


def check_render(got, want, where, vibrato=False):
    assert same_bits(got["owner"], want["owner"]), (where, "owner")
    if vibrato:
        assert got["position"].dtype == np.int64 and np.abs(got["position"] - want["position"]).max() <= 1, (where, "position")
    else:
        assert same_bits(got["position"], want["position"]), (where, "position")
    cents, f0 = nref.controls_of(got["position"] if vibrato else want["position"])
    assert same_bits(got["cents"], cents), (where, "cents")
    assert within_one_ulp(got["f0"], f0), (where, "f0")
    assert within_one_ulp(got["loudness"], want["loudness"]), (where, "loudness")
    assert same_bits(got["harmonicity"], want["harmonicity"]) and same_bits(got["voiced"], want["voiced"]), where


def run_render_case(rec, offset, T, device, options, where):
    want = nref.render(rec, offset, T, **loop_options(options))
    got = got_render(notes_of(rec, offset, device), T, **options)
    check_render(got, want, (where, options), vibrato="vibrato_cents" in options)
    return want


def run_render_cases(T, device, sizes=RENDER_N):
    for j, N in enumerate(sizes):
        B = 3
        rec = make_records(200 + T + N, B, N, T)
        offset = [(-50, 0, 37)[(b + N) % 3] for b in range(B)] if N % 2 else [13]      # G = B and G = 1
        picks = RENDER_OPTIONS if (T, N) == (172, 65) else [RENDER_OPTIONS[(3 * j + T + i) % len(RENDER_OPTIONS)] for i in range(3)] + \
            [RENDER_OPTIONS[12 + (T + j) % 5]]
        for options in picks:
            want = run_render_case(rec, offset, T, device, options, (T, N))
        if N >= 64 and T >= 63:
            assert (want["owner"] >= 0).any() and (want["owner"] < 0).any()


@pytest.mark.parametrize("T", RENDER_T)
def test_cpu_render_equals_plain_loops(T):
    run_render_cases(T, "cpu")


def designed_records(T):
    """One row per situation the definition names (T >= 40)."""
    rows = [
        # a note that starts before frame 0 and one that ends after T; a note that starts at T
        [(-5, 12, 60), (T - 4, 30, 64), (T, 5, 67)],
        # overlapping notes (the later one cuts), two notes with equal onsets (the earlier one owns nothing)
        [(2, 20, 60), (10, 20, 62), (15, 9, 65), (15, 6, 67)],
        # touching notes (legato) and notes with gaps
        [(0, 8, 60), (8, 8, 62), (16, 8, 64), (30, 4, 65), (36, 3, 72)],
        # invalid records in the middle: frames = 0, pitch = INT32_MIN, pitch = 128
        [(1, 6, 60), (7, 0, 62), (12, 5, nref.NO_PITCH), (17, 5, 128), (22, 6, 64), (28, 6, 65)],
        # a row whose first note is invalid (nothing to hold before it), and a row with count = 0
        [(5, 0, 60), (9, 4, 62)],
        [(3, 5, 60), (9, 5, 62)],
    ]
    N = max(len(r) for r in rows)
    rec = dict(onset=np.full((len(rows), N), -1, np.int32), frames=np.zeros((len(rows), N), np.int32),
               pitch=np.full((len(rows), N), nref.NO_PITCH, np.int32), detune=np.zeros((len(rows), N), np.int32),
               level=np.full((len(rows), N), np.nan, np.float32), count=np.array([len(r) for r in rows], dtype=np.int32))
    rng = np.random.default_rng(174)
    for b, row in enumerate(rows):
        for i, (s, L, p) in enumerate(row):
            rec["onset"][b, i], rec["frames"][b, i], rec["pitch"][b, i] = s, L, p
            rec["detune"][b, i] = rng.integers(-30 * 65536, 30 * 65536)
            rec["level"][b, i] = np.nan if i % 3 == 1 else rng.random()                  # NaN levels
    rec["count"][5] = 0
    return rec


def check_designed_render(device):
    T = 44
    rec = designed_records(T)
    for options in RENDER_OPTIONS:
        want = run_render_case(rec, [21], T, device, options, "designed")
    want = nref.render(rec, [21], T)
    owner = want["owner"]
    assert owner[0, 0] == 0 and owner[0, 6] == 0 and owner[0, 7] == -1 and owner[0, T - 1] == 1          # before 0, past T, starts at T
    assert owner[1, 9] == 0 and owner[1, 10] == 1 and owner[1, 14] == 1 and (owner[1] != 2).all() and owner[1, 20] == 3 and owner[1, 21] == -1
    assert owner[2, 7] == 0 and owner[2, 8] == 1 and owner[2, 24] == -1 and owner[2, 30] == 3
    assert (owner[3, 7:22] == -1).all() and owner[3, 6] == 0 and owner[3, 22] == 4
    assert want["position"][4, 0] == nref.HOLD and want["position"][4, 6] == nref.HOLD and owner[4, 9] == 1
    assert (owner[5] == -1).all() and (want["position"][5] == nref.HOLD).all() and (want["loudness"][5] == 0).all()
    assert want["position"][3, 9] == nref.HOLD != want["position"][3, 5]        # an invalid note cuts the one before it, and holds nothing
    assert want["position"][2, 25] == 64 * ref.S + 21 * 65536 + int(rec["detune"][2, 2])     # off frames hold the pitch of the note before


def test_designed_note_lists():
    check_designed_render("cpu")


# ------------------------------------------------------------------------------------------------------------------ round trip
def score(seed, B, N, root, min_note=1):
    """sorted, non-overlapping notes on the major scale of `root`, no two touching notes of equal pitch"""
    rng = np.random.default_rng(seed)
    degrees = [0, 2, 4, 5, 7, 9, 11]
    onset, frames, pitch = np.zeros((B, N), np.int32), np.zeros((B, N), np.int32), np.zeros((B, N), np.int32)
    T = 0
    for b in range(B):
        at, last = int(rng.integers(0, 4)), -1
        for i in range(N):
            onset[b, i], frames[b, i] = at, rng.integers(min_note, min_note + 9)
            while True:
                p = 48 + root + 12 * int(rng.integers(0, 3)) + degrees[int(rng.integers(0, 7))]
                if p != last:
                    break
            pitch[b, i] = last = p
            at += int(frames[b, i]) + (0 if rng.random() < 0.5 else int(rng.integers(1, 6)))      # touching, or a gap
        T = max(T, at)
    return dict(onset=onset, frames=frames, pitch=pitch, count=np.full(B, N, np.int32)), T


def check_round_trip(device):
    for seed, min_note, with_detune in ((181, 1, False), (182, 3, False), (183, 1, True), (184, 2, True)):
        B, N, root, offset = 3, 40, 2, [-17, 0, 33]
        rec, T = score(seed, B, N, root, min_note)
        rng = np.random.default_rng(seed)
        rec["detune"] = rng.integers(-30 * 65536 + 1, 30 * 65536, (B, N)).astype(np.int32) if with_detune else np.zeros((B, N), np.int32)
        rec["level"] = rng.random((B, N)).astype(np.float32)
        # the preconditions, on the test's own input
        nxt = np.concatenate([rec["onset"][:, 1:], np.full((B, 1), T, np.int32)], axis=1)
        assert (np.diff(rec["onset"], axis=1) > 0).all() and (rec["onset"] + rec["frames"] <= nxt).all()
        assert (np.minimum(rec["frames"], nxt - rec["onset"]) >= max(1, min_note)).all()
        assert all(ref.allowed(int(p), root, 0xAB5) for p in rec["pitch"].reshape(-1))
        touching = rec["onset"][:, :-1] + rec["frames"][:, :-1] == rec["onset"][:, 1:]
        assert touching.any() and (~touching).any() and (rec["pitch"][:, :-1] != rec["pitch"][:, 1:])[touching].all()
        assert (np.abs(rec["detune"]) < 30 * 65536).all()
        notes = notes_of(rec, offset, device, root=[root] * B, scale="major")
        z = render_notes(notes, T, SR, HOP, detune=with_detune, glide=0, vibrato_cents=0.0)
        back = extract_notes(z, notes.tuning(), hysteresis=20.0, min_note_frames=min_note, max_notes=N)
        got = records_of(back)
        for k in ("count", "onset", "frames", "pitch"):
            assert same_bits(got[k], rec[k]), (seed, k)
        assert same_bits(got["level"], rec["level"])                            # a note's level comes back as well: no attack, no release
        cents = z["normalized_cents"].cpu().numpy().reshape(B, T)
        for b in range(B):
            for i in range(N):
                bound = 65536.0 * 7180.0 * float(np.spacing(np.abs(cents[b, rec["onset"][b, i]]))) / 2.0 + 1.0
                assert abs(int(got["detune"][b, i]) - int(rec["detune"][b, i])) <= bound, (seed, b, i, got["detune"][b, i], bound)


def test_round_trip():
    check_round_trip("cpu")


def check_melody(device):
    cents, played = ref.melody()
    z = z_of(dict(cents=cents, f0=ref.f0_of_cents(cents)), device, keys=("cents", "f0"))
    stats = tuning_statistics(z)
    notes = extract_notes(z, stats, hysteresis=20.0)
    frame_notes, _ = nref.expand(records_of(notes), 860)
    assert np.array_equal(frame_notes[0], played) and notes.validate() is notes
    o = int(stats.offset[0])
    out = render_notes(notes, 860, SR, HOP, detune=False, return_info=True)
    n2, owner = out["normalized_cents"].cpu().numpy().reshape(-1), out["owner"].cpu().numpy().reshape(-1)
    assert (owner >= 0).all()
    for t in range(860):
        bound = 7180 * Fraction(float(np.spacing(np.abs(n2[t])))) / 2 + Fraction(1, 1 << 17)
        assert abs(7180 * Fraction(float(n2[t])) + Fraction(ref.K) - (100 * int(played[t]) + o)) <= bound, t


def test_melody_recovered_and_rendered():
    check_melody("cpu")


# ------------------------------------------------------------------------------------------------------------------ the edits
def loop_degrees(pitch, k, root, mask):
    step = 1 if k > 0 else -1
    for _ in range(abs(k)):
        pitch += step
        while not ref.allowed(pitch, root, mask):
            pitch += step
    return pitch


def test_transpose_and_transpose_degrees():
    rec, _ = score(191, 2, 30, 0)
    rec["detune"], rec["level"] = np.zeros((2, 30), np.int32), np.zeros((2, 30), np.float32)
    rec["count"][1] = 20
    rec["pitch"][1, 20:] = nref.NO_PITCH
    for name, mask in ref.SCALES.items():
        for roots in ([0], [3, 10]):
            notes = notes_of(rec, [0] * len(roots), "cpu", root=roots, scale=name)
            there = notes.transpose(12).transpose(-12)
            assert all(torch.equal(getattr(there, k), getattr(notes, k)) for k in RECORDS)
            assert torch.equal(notes.transpose(12).pitch[0], notes.pitch[0] + 12) and int(notes.transpose(12).pitch[1, 25]) == nref.NO_PITCH
            for k in (-8, -1, 0, 1, 2, 7):
                moved = notes.transpose_degrees(k)
                assert moved is not notes and torch.equal(moved.onset, notes.onset)
                for b in range(2):
                    r = roots[b if len(roots) > 1 else 0]
                    for i in range(30):
                        p = int(notes.pitch[b, i])
                        if p == nref.NO_PITCH:
                            assert int(moved.pitch[b, i]) == nref.NO_PITCH
                            continue
                        want = loop_degrees(p, k, r, mask)
                        assert int(moved.pitch[b, i]) == want and (k == 0 or ref.allowed(want, r, mask)), (name, roots, k, b, i)
    major = notes_of(rec, [0], "cpu", root=[0], scale="major")              # the score is in C major: seven degrees are an octave
    assert torch.equal(major.transpose_degrees(7).pitch, major.transpose(12).pitch)
    part = major.transpose(2.25)                                             # a fraction goes into detune
    assert torch.equal(part.pitch[0], major.pitch[0] + 2) and set(part.detune[0].tolist()) == {ref.S // 4}
    with pytest.raises(ValueError):
        major.transpose_degrees(1.5)


def test_quantize_and_sorted():
    onset = [[0, 1, 2, 3, 5, 6, 7, 9, 10, 11, 14, 21, 22, 23]]
    notes = Notes(onset=onset, frames=[[2] * 14], pitch=[list(range(60, 74))], count=[12])
    for g in (1, 4, 7):
        q = notes.quantize(g)
        want = [-(-(2 * o - g) // (2 * g)) * g for o in onset[0][:12]]          # ceil((o - g / 2) / g): the nearest line, ties down
        assert q.onset[0, :12].tolist() == want and q.onset[0, 12:].tolist() == onset[0][12:], (g, q.onset)
        assert all(abs(w - o) * 2 <= g for w, o in zip(want, onset[0])) and want == sorted(want)
        assert torch.equal(q.frames, notes.frames) and torch.equal(q.pitch, notes.pitch)
    assert notes.quantize(4).onset[0, :8].tolist() == [0, 0, 0, 4, 4, 4, 8, 8]  # 2 and 6 are ties: down
    with pytest.raises(ValueError):
        notes.quantize(0)
    mixed = Notes(onset=[[9, 3, 3, 1, 50]], frames=[[1, 2, 3, 4, 5]], pitch=[[60, 61, 62, 63, 64]], count=[4])
    with pytest.raises(ValueError):
        mixed.validate()
    s = mixed.sorted()
    assert s.onset.tolist() == [[1, 3, 3, 9, 50]] and s.frames.tolist() == [[4, 2, 3, 1, 5]] and s.validate() is s


# ------------------------------------------------------------------------------------------------------------------ MIDI files
def test_midi_round_trip(tmp_path):
    sr, hop = 48000, 100                                        # 960 ticks a second: a frame is 2 ticks
    assert Fraction(hop * 960, sr).denominator == 1
    rec, T = score(195, 1, 25, 0, 2)
    rng = np.random.default_rng(195)
    step = 3.0 / 127.0                                          # levels from velocity 1 up: below it the velocity is clamped
    level = (-2.0 + step + rng.random((1, 25)) * (3.0 - step)).astype(np.float32)
    level[0, 3] = np.nan
    notes = Notes(rec["onset"], rec["frames"], rec["pitch"], detune=rng.integers(-999, 999, (1, 25)), level=level)
    path = str(tmp_path / "score.mid")
    notes.write_midi(path, hop, sr, level_range=(-2.0, 1.0))
    back = Notes.read_midi(path, hop, sr, level_range=(-2.0, 1.0))
    for k in ("onset", "frames", "pitch"):
        assert torch.equal(getattr(back, k), getattr(notes, k)), k
    assert int(back.count[0]) == 25 and not back.detune.any() and back.mask == 0xFFF
    want = np.where(np.isnan(level[0]), -2.0 + 64 * step, level[0])
    assert np.abs(back.level[0].numpy() - want).max() <= step / 2 + 1e-6
    # an overlap is written as the render plays it: the later note cuts the earlier one
    Notes(onset=[0, 4], frames=[10, 3], pitch=[60, 62], level=[2.0, -1.0]).write_midi(path, hop, sr)
    cut = Notes.read_midi(path, hop, sr)
    assert cut.onset.tolist() == [[0, 4]] and cut.frames.tolist() == [[4, 3]] and np.allclose(cut.level.numpy(), [[1.0, 1.0 / 127.0]], atol=1e-7)


def vlq(n):
    out = [n & 0x7F]
    n >>= 7
    while n:
        out.append(0x80 | (n & 0x7F))
        n >>= 7
    return bytes(reversed(out))


def chunk(kind, body):
    return kind + struct.pack(">I", len(body)) + body


def test_midi_by_hand(tmp_path):
    """format 1, two tracks, running status, a tempo change, a velocity-0 note-off; 96 ticks per quarter.
    At 500000 us per quarter a tick is 1/192 s; from tick 192 on, at 250000, 1/384 s.  hop 125 at 48 kHz: 384 frames a second."""
    sr, hop = 48000, 125
    tempo = bytes([0x00, 0xFF, 0x51, 0x03]) + (500000).to_bytes(3, "big") + vlq(192) + bytes([0xFF, 0x51, 0x03]) + (250000).to_bytes(3, "big") + \
        bytes([0x00, 0xFF, 0x2F, 0x00])
    notes = (bytes([0x00, 0xFF, 0x03, 0x02]) + b"hi"                         # a track name: ignored
             + bytes([0x00, 0xC0, 0x05])                                      # a program change: one data byte
             + bytes([0x00, 0x90, 60, 100])                                   # tick 0: note 60 on
             + vlq(96) + bytes([60, 0])                                       # tick 96, running status: velocity 0 is a note-off
             + vlq(0) + bytes([62, 80])                                       # tick 96, running status: note 62 on
             + vlq(48) + bytes([0xB0, 7, 90])                                 # tick 144: a controller, ignored
             + vlq(48) + bytes([0x90, 64, 127])                               # tick 192: note 64 on cuts note 62
             + vlq(96) + bytes([0x80, 62, 0])                                 # tick 288: the off of a note that no longer sounds
             + vlq(96) + bytes([0x80, 64, 64])                                # tick 384: note 64 off
             + bytes([0x00, 0xF0, 0x02, 0x01, 0xF7])                          # a system-exclusive message, ignored
             + vlq(0) + bytes([0x99, 36, 1]) + vlq(384) + bytes([36, 0])      # tick 384 .. 768: note 36 on another channel
             + bytes([0x00, 0xFF, 0x2F, 0x00]))
    path = str(tmp_path / "hand.mid")
    with open(path, "wb") as f:
        f.write(chunk(b"MThd", struct.pack(">HHH", 1, 2, 96)) + chunk(b"MTrk", tempo) + chunk(b"MTrk", notes))
    got = Notes.read_midi(path, hop, sr)
    # seconds: 0, 0.5, 1.0, then half as long per tick: 1.5, 2.5
    assert got.onset.tolist() == [[0, 192, 384, 576]] and got.frames.tolist() == [[192, 192, 192, 384]]
    assert got.pitch.tolist() == [[60, 62, 64, 36]] and got.count.tolist() == [4]
    assert np.allclose(got.level[0].numpy(), np.array([100, 80, 127, 1]) / 127.0, atol=1e-7)
    with open(path, "wb") as f:
        f.write(chunk(b"MThd", struct.pack(">HHh", 0, 1, -(25 << 8) + 40)) + chunk(b"MTrk", tempo))
    with pytest.raises(ValueError, match="SMPTE"):
        Notes.read_midi(path, hop, sr)
    with open(path, "wb") as f:
        f.write(b"RIFF" + bytes(20))
    with pytest.raises(ValueError):
        Notes.read_midi(path, hop, sr)


# ------------------------------------------------------------------------------------------------------------------ wiring, ABI
def test_notes_object_and_errors():
    n = Notes(onset=[0, 10], frames=[10, 8], pitch=[60, 62])
    assert (n.rows, n.max_notes, n.groups) == (1, 2) + (1,) and n.count.tolist() == [2] and not n.detune.any() and bool(n.level.isnan().all())
    assert n.offset.tolist() == [0] and n.root.tolist() == [0] and n.mask == 0xAB5 and n.source_frames is None
    d = n.to_dict()
    m = Notes.from_dict(d).to("cpu")
    assert all(same_bits(getattr(m, k).numpy(), getattr(n, k).numpy()) for k in RECORDS + ("offset", "root")) and m.options() == n.options()
    assert Notes([[1, 2], [3, 4]], [[1, 1], [1, 1]], [[60, 61], [62, 63]], offset=[3, -4], root=[0, 11], scale=0x091).groups == 2
    for bad in (dict(onset=[0], frames=[1, 2], pitch=[60]), dict(onset=[0], frames=[1], pitch=[60], offset=51),
                dict(onset=[0], frames=[1], pitch=[60], root=12), dict(onset=[0], frames=[1], pitch=[60], count=[1, 2]),
                dict(onset=[0], frames=[1], pitch=[60], offset=[0, 0, 0], root=[0, 0, 0]), dict(onset=[0], frames=[1], pitch=[60], scale="lydian")):
        with pytest.raises(ValueError):
            Notes(**bad)
    x = ref.make(144, 2, 9)
    z = z_of(x)
    for bad in (dict(hysteresis=-1.0), dict(hysteresis=1201.0), dict(min_note_frames=-1), dict(max_notes=-1), dict(max_notes=1.5),
                dict(scale=0), dict(root=12), dict(tuning=3), dict(tuning=TuningStatistics([0, 0, 0], [0, 0, 0]))):
        with pytest.raises(ValueError):
            extract_notes(z, **bad)
    with pytest.raises(ValueError):
        extract_notes({"harmonicity": z["harmonicity"]})
    with pytest.raises(Exception, match="grad"):
        extract_notes(dict(z, normalized_cents=z["normalized_cents"].clone().requires_grad_()))
    with pytest.raises(Exception, match="grad"):
        extract_notes(dict(z, loudness=z["loudness"].clone().requires_grad_()))
    own = extract_notes(z)                                      # tuning=None: each row measured by itself
    stats = tuning_statistics(z, per_row=True)
    assert torch.equal(own.offset, stats.offset) and torch.equal(own.root, stats.root) and own.max_notes == 9
    assert all(same_bits(getattr(own, k).numpy(), getattr(extract_notes(z, stats), k).numpy()) for k in RECORDS)
    assert extract_notes(z, min_note_frames=4).max_notes == 2
    for bad in (dict(frames=0), dict(glide=-1), dict(attack=1.5), dict(release=-2), dict(vibrato_ramp=0), dict(vibrato_delay=-1),
                dict(transpose=200.0), dict(vibrato_cents=-1.0), dict(floor=float("nan")), dict(default_level=float("inf")), dict(glide=1 << 24)):
        with pytest.raises(ValueError):
            render_notes(n, **dict(dict(frames=20, sample_rate=SR, hop_length=HOP), **bad))
    with pytest.raises(ValueError):
        render_notes(z, 20, SR, HOP)
    with pytest.raises(Exception, match="grad"):
        render_notes(Notes(n.onset, n.frames, n.pitch, level=torch.zeros(1, 2, requires_grad=True)), 20, SR, HOP)


def test_symbols_and_entry_point_validation():
    names = list(declared_prototypes())
    L = ctypes.CDLL(ddsp._lib.SO_PATH)
    for name in NEW_SYMBOLS:
        assert name in ddsp._lib.EXPORTS and name in ddsp._lib.SIGNATURES and hasattr(L, name), name
    # the last additions but one: tests/test_trainer_host.py keeps ddsp_gather_batch the last symbol of the table
    around = ("ddsp_griffinlim_stage",) + NEW_SYMBOLS + ("ddsp_gather_batch",)
    assert tuple(names[-4:]) == around == tuple(ddsp._lib.SIGNATURES)[-4:] == ddsp._lib.EXPORTS[-4:]
    assert ddsp._lib.ABI_VERSION == 5 == ddsp._lib.lib().ddsp_hip_abi_version()
    assert ddsp.extract_notes is extract_notes and ddsp.render_notes is render_notes and ddsp.Notes is Notes
    assert {"notes", "Notes", "extract_notes", "render_notes"} <= set(ddsp.__all__)
    assert hasattr(ddsp.AutoEncoder, "transcribe") and hasattr(ddsp.AutoEncoder, "play")
    assert ddsp.notes.NO_PITCH == nref.NO_PITCH and ddsp.notes.HOLD == nref.HOLD and ddsp.notes.MAX_DETUNE == nref.MAX_DETUNE
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ddsp_hip.h")).read()
    assert "#define DDSP_HIP_ABI_VERSION 5" in header and "#define DDSP_NOTES_KEEP_DETUNE 1" in header and "#define DDSP_NOTES_CONCERT 2" in header
    L = ddsp._lib.lib()
    EINVAL, ERANGE = -1, -2
    word = (ctypes.c_uint64 * 8)()
    p = ctypes.addressof(word)

    def extract(B=1, T=5, N=3, groups=1, mask=0xAB5, root=-1, h=0, min_note=0, gate=0, silence=0.0, confidence=0.0, cents=p, loud=None,
                count=p, onset=p):
        return L.ddsp_notes_extract(cents, None, loud, None, p, p, onset, p, p, p, p, count, B, T, N, groups, mask, root, h, min_note, gate,
                                    silence, confidence, None)

    assert extract(B=0) == 0 and extract(B=-1) == EINVAL and extract(T=0) == EINVAL and extract(N=-1) == EINVAL
    assert extract(mask=0) == EINVAL and extract(mask=0x1000) == EINVAL and extract(root=12) == EINVAL and extract(root=-2) == EINVAL
    assert extract(h=-1) == EINVAL and extract(h=1200 * 65536 + 1) == EINVAL and extract(min_note=-1) == EINVAL
    assert extract(silence=float("nan")) == EINVAL and extract(confidence=float("nan")) == EINVAL and extract(gate=2) == EINVAL
    assert extract(gate=1) == EINVAL and extract(cents=None) == EINVAL and extract(count=None) == EINVAL and extract(onset=None) == EINVAL
    assert extract(B=3, groups=2) == EINVAL
    assert extract(T=1 << 24) == ERANGE and extract(B=1 << 12, T=1 << 19, N=0) == ERANGE and extract(B=1 << 12, T=5, N=1 << 19) == ERANGE

    def render(B=1, T=5, N=3, groups=1, flags=1, transpose=0, glide=0, attack=0, release=0, delay=0, ramp=1, depth=0.0, omega=0.0, floor=0.0,
               default=1.0, onset=p, count=p, f0=p, voiced=p):
        return L.ddsp_notes_render(onset, p, p, p, p, count, p, f0, p, p, p, voiced, None, None, B, T, N, groups, flags, transpose, glide, attack,
                                   release, delay, ramp, depth, omega, floor, default, None)

    assert render(B=0) == 0 and render(B=-1) == EINVAL and render(T=0) == EINVAL and render(N=-1) == EINVAL and render(flags=4) == EINVAL
    assert render(transpose=128 * ref.S + 1) == EINVAL and render(transpose=-128 * ref.S - 1) == EINVAL
    assert render(glide=-1) == EINVAL and render(glide=1 << 24) == EINVAL and render(attack=-1) == EINVAL and render(release=1 << 24) == EINVAL
    assert render(delay=-1) == EINVAL and render(ramp=0) == EINVAL and render(ramp=1 << 24) == EINVAL
    assert render(depth=-1.0) == EINVAL and render(depth=float("nan")) == EINVAL and render(omega=float("nan")) == EINVAL
    assert render(floor=float("nan")) == EINVAL and render(default=float("inf")) == EINVAL
    assert render(onset=None) == EINVAL and render(count=None) == EINVAL and render(f0=None) == EINVAL and render(voiced=None) == EINVAL
    assert render(B=3, groups=2) == EINVAL
    assert render(T=1 << 24) == ERANGE and render(B=1 << 12, T=1 << 19, N=0) == ERANGE and render(B=1 << 12, T=5, N=1 << 19) == ERANGE
