"""Polyphony on the CPU path (voices.py) against the plain loops of tests/voices_reference.py: the
allocation to the bit in every output, the mix within (V + 6) 2^-24 of the sum of the terms' magnitudes (the count of the
roundings stands in voices_reference.py), chords through MIDI files, the wiring of the two entry points and the refusals.
tests/test_gpu_voices.py runs the same cases on the device; the reference of a case is computed once and shared."""
import ctypes
import functools
import os
import struct

import numpy as np
import pytest
import torch

import ddsp_pytorch_amd as ddsp
import voices_reference as vref
from ddsp_pytorch_amd import voices
from ddsp_pytorch_amd.notes import Notes, render_notes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORDS = ("onset", "frames", "pitch", "detune", "level")
VOICE_KEYS = RECORDS + ("count", "index", "voice", "slot", "stolen", "dropped")
ASSIGNS, STEALS = tuple(vref.ASSIGN), tuple(vref.STEAL)
NAN = np.float32(np.nan)


# ------------------------------------------------------------------------------------------------------------------ allocation
def random_score(seed, B=3, N=40, clean=False):
    """Scores whose notes overlap, onsets in order; unless `clean` (every note valid, no two of one onset), some notes that sound
    nowhere, some levels missing and one count beyond N."""
    rng = np.random.default_rng(seed)
    onset = np.cumsum(rng.integers(1 if clean else 0, 4, (B, N)), axis=1).astype(np.int32)
    frames = rng.integers(1, 14, (B, N)).astype(np.int32)
    pitch = rng.integers(48, 84, (B, N)).astype(np.int32)
    detune = rng.integers(-400000, 400000, (B, N)).astype(np.int32)
    level = rng.standard_normal((B, N)).astype(np.float32)
    count = np.full(B, N, dtype=np.int32)
    if not clean:
        bad = rng.random((B, N)) < 0.08
        kind = rng.integers(0, 4, (B, N))
        frames[bad & (kind == 0)] = rng.choice([0, -3])
        pitch[bad & (kind == 1)] = rng.choice([-1, 128, vref.NO_PITCH])
        detune[bad & (kind == 2)] = (1 << 30) + 1
        level[rng.random((B, N)) < 0.2] = NAN
        level[:, 3:4] = -0.0
        count[:] = [N - 7, N + 3, N][:B] + [N] * max(0, B - 3)
    return dict(onset=onset, frames=frames, pitch=pitch, detune=detune, level=level, count=count)


def score(rows, count=None):
    """hand-made rows of (onset, frames, pitch[, level[, detune]]) tuples -> records"""
    N = max(len(r) for r in rows)
    rec = dict(onset=np.full((len(rows), N), -1, np.int32), frames=np.zeros((len(rows), N), np.int32),
               pitch=np.full((len(rows), N), vref.NO_PITCH, np.int32), detune=np.zeros((len(rows), N), np.int32),
               level=np.full((len(rows), N), NAN, np.float32))
    for b, row in enumerate(rows):
        for i, note in enumerate(row):
            rec["onset"][b, i], rec["frames"][b, i], rec["pitch"][b, i] = note[:3]
            rec["level"][b, i] = note[3] if len(note) > 3 else NAN
            rec["detune"][b, i] = note[4] if len(note) > 4 else 0
    rec["count"] = np.array([len(r) for r in rows] if count is None else count, dtype=np.int32)
    return rec


def notes_of(rec, device, **options):
    return Notes(*(torch.from_numpy(rec[k]) for k in RECORDS), torch.from_numpy(rec["count"]), scale="chromatic", **options).to(device)


def want_alloc(rec, V, Nv, assign, steal, gap):
    rows = [vref.allocate_row(*(rec[k][b].tolist() for k in RECORDS), int(rec["count"][b]), V, Nv, vref.ASSIGN[assign], vref.STEAL[steal], gap)
            for b in range(rec["onset"].shape[0])]
    B, N = rec["onset"].shape
    out = {k: np.array([r[k] for r in rows], dtype=np.float32 if k == "level" else np.int32) for k in VOICE_KEYS}
    for k in RECORDS + ("index",):
        out[k] = out[k].reshape(B * V, Nv)
    out["count"] = out["count"].reshape(B * V)
    out["voice"], out["slot"] = out["voice"].reshape(B, N), out["slot"].reshape(B, N)
    return out


def got_alloc(rec, device, V, Nv, assign, steal, gap):
    found, info = voices.allocate_voices(notes_of(rec, device), V, assign=assign, steal=steal, gap=gap, max_notes=Nv, return_info=True)
    out = {k: getattr(found, k).cpu().numpy() for k in RECORDS + ("count",)}
    out.update({k: v.cpu().numpy() for k, v in info.items()})
    return out


def bits(x):
    return x.view(np.uint32) if x.dtype == np.float32 else x


def check_alloc(got, want, what):
    for k in VOICE_KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape, want[k].shape)
        assert np.array_equal(bits(got[k]), bits(want[k])), (what, k)


@functools.lru_cache(maxsize=None)
def random_case(V, assign, steal, gap):
    """(records, Nv, the loops' answer) of the random scores for one setting, computed once for the CPU and the device tests"""
    rec = random_score(1000 + V)
    Nv = 40 if V < 4 else 12
    return rec, Nv, want_alloc(rec, V, Nv, assign, steal, gap)


ALLOC_SETTINGS = [(V, a, s, gap) for V in (1, 2, 4, 64) for a in ASSIGNS for s in STEALS for gap in (0, 3)]


def run_random_allocation(device):
    fired = dict(stolen=0, dropped=0, overflow=0, skipped=0)
    for V, assign, steal, gap in ALLOC_SETTINGS:
        rec, Nv, want = random_case(V, assign, steal, gap)
        check_alloc(got_alloc(rec, device, V, Nv, assign, steal, gap), want, (V, assign, steal, gap))
        fired["stolen"] += int(want["stolen"].sum())
        fired["dropped"] += int(want["dropped"].sum())
        fired["overflow"] += int((want["count"] > Nv).sum())
        fired["skipped"] += int((want["voice"] == -1).sum())
    assert all(v > 0 for v in fired.values()), fired


def check_designed_allocation(device):
    """hand-made scores in which each rule fires by construction"""
    run = lambda rec, V, assign, steal, gap=0, Nv=None: _designed(rec, device, V, Nv or rec["onset"].shape[1], assign, steal, gap)  # noqa: E731
    # five notes of one onset on four voices: one steal (of voice 0, whose note keeps 0 frames), or one drop
    five = score([[(0, 10, 60 + i) for i in range(5)]])
    got = run(five, 4, "lowest", "oldest")
    assert got["stolen"].tolist() == [1] and got["dropped"].tolist() == [0] and got["voice"].tolist() == [[0, 1, 2, 3, 0]]
    assert got["frames"][0, :2].tolist() == [0, 10] and got["slot"].tolist() == [[0, 0, 0, 0, 1]] and got["count"].tolist() == [2, 1, 1, 1]
    got = run(five, 4, "lowest", "drop")
    assert got["stolen"].tolist() == [0] and got["dropped"].tolist() == [1] and got["voice"].tolist() == [[0, 1, 2, 3, -1]]
    assert got["count"].tolist() == [1, 1, 1, 1] and got["frames"][:, 0].tolist() == [10] * 4
    # C-E-G then A-F-D: under 'nearest' each voice moves by a step, whatever the order of the second chord; 'lowest' takes the order
    chords = score([[(0, 10, 60), (0, 10, 64), (0, 10, 67), (10, 10, 69), (10, 10, 65), (10, 10, 62)]])
    assert run(chords, 3, "nearest", "oldest")["voice"].tolist() == [[0, 1, 2, 2, 1, 0]]
    assert run(chords, 3, "lowest", "oldest")["voice"].tolist() == [[0, 1, 2, 0, 1, 2]]
    assert run(chords, 3, "nearest", "oldest", gap=1)["stolen"].tolist() == [3]      # (a gap of one frame: no voice is free yet)
    # a re-struck pitch returns to its voice; round robin takes the voice that has rested longest
    again = score([[(0, 5, 60), (0, 8, 72), (20, 5, 72), (30, 5, 50)]])
    assert run(again, 2, "nearest", "oldest")["voice"].tolist() == [[0, 1, 1, 0]]
    assert run(again, 2, "lowest", "oldest")["voice"].tolist() == [[0, 1, 0, 0]]
    assert run(again, 2, "oldest", "oldest")["voice"].tolist() == [[0, 1, 0, 1]]
    # two levels and a note without one under 'quietest': the note without a level survives
    levels = score([[(0, 10, 60), (0, 10, 62, 0.5), (5, 10, 64, 0.9), (6, 10, 65, -2.0)]])
    got = run(levels, 2, "lowest", "quietest")
    assert got["voice"].tolist() == [[0, 1, 1, 1]] and got["stolen"].tolist() == [2] and got["frames"][0, 0] == 10
    assert got["frames"][1, :3].tolist() == [5, 1, 10]
    assert run(levels, 2, "lowest", "oldest")["voice"].tolist() == [[0, 1, 0, 1]]
    # four notes on one voice of two slots: count 4, two written
    line = score([[(0, 5, 60), (5, 5, 62), (10, 5, 64), (15, 5, 65)]])
    got = run(line, 1, "nearest", "oldest", Nv=2)
    assert got["count"].tolist() == [4] and got["slot"].tolist() == [[0, 1, -1, -1]] and got["voice"].tolist() == [[0, 0, 0, 0]]
    assert got["pitch"].tolist() == [[60, 62]] and got["index"].tolist() == [[0, 1]]
    # notes that sound nowhere are skipped and free no voice
    bad = score([[(0, 10, 60), (0, 0, 61), (-1, 5, 62), (1, 5, 128), (2, 5, 63, 1.0, (1 << 30) + 1), (3, 5, 64, 1.0, -(1 << 30))]])
    got = run(bad, 2, "lowest", "drop")
    assert got["voice"].tolist() == [[0, -1, -1, -1, -1, 1]] and got["dropped"].tolist() == [0] and got["index"][1, 0] == 5
    # a count beyond N is N, a negative one 0
    got = run(score([[(0, 5, 60), (5, 5, 62)], [(0, 5, 60), (5, 5, 62)]], count=[7, -2]), 2, "lowest", "oldest")
    assert got["count"].tolist() == [2, 0, 0, 0] and got["voice"].tolist() == [[0, 0], [-1, -1]]


def _designed(rec, device, V, Nv, assign, steal, gap):
    got = got_alloc(rec, device, V, Nv, assign, steal, gap)
    check_alloc(got, want_alloc(rec, V, Nv, assign, steal, gap), (V, Nv, assign, steal, gap))
    return got


def check_one_voice_renders_as_the_source(device):
    """V = 1 with 'oldest' stealing is the monophonic instrument: the voice row renders as the source does, to the bit (valid notes
    of distinct onsets: a note the steal leaves 0 frames would no longer count as the one a glide starts from)"""
    rec = random_score(77, B=3, N=30, clean=True)
    source = notes_of(rec, device)
    row, info = voices.allocate_voices(source, 1, assign="lowest", steal="oldest", return_info=True)
    assert int(info["stolen"].sum()) > 10 and bool((info["dropped"] == 0).all())
    options = dict(glide=2, attack=2, release=3, vibrato_cents=20.0, return_info=True)
    a, b = render_notes(source, 90, 44100, 512, **options), render_notes(row, 90, 44100, 512, **options)
    for k in a:
        x, y = a[k].cpu().numpy(), b[k].cpu().numpy()
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), k
    assert int(a["voiced"].sum()) > 100


def test_allocation_equals_plain_loops():
    run_random_allocation("cpu")


def test_designed_scores_fire_every_rule():
    check_designed_allocation("cpu")


def test_one_voice_is_the_monophonic_instrument():
    check_one_voice_renders_as_the_source("cpu")


def test_allocated_notes_carry_the_tuning_and_the_options():
    rec = random_score(5, B=2, N=6, clean=True)
    per_row = notes_of(rec, "cpu", offset=torch.tensor([3, -7], dtype=torch.int32), root=torch.tensor([2, 9], dtype=torch.int32),
                       source_frames=123, silence=-4.0, confidence=0.25)
    found = voices.allocate_voices(per_row, 3)
    assert found.rows == 6 and found.max_notes == 6 and found.offset.tolist() == [3, 3, 3, -7, -7, -7] and found.root.tolist() == [2, 2, 2, 9, 9, 9]
    assert found.options() == per_row.options() and found.source_frames == 123
    shared = voices.allocate_voices(notes_of(rec, "cpu", offset=4, root=1), 3, max_notes=2)
    assert shared.groups == 1 and shared.offset.tolist() == [4] and shared.max_notes == 2 and shared.rows == 6


# ------------------------------------------------------------------------------------------------------------------ the mix
HOP = 64
MIX_SHAPES = [(V, C, L) for V in (1, 3, 64) for C in (1, 2) for L in (1, 63, 64, 67, 4 * 172 + 3)]
GATES = [None, (0, 0, "above"), (0, 5, "below"), (2, 3, "above")]       # hold, fade, T hop above or below L
# beyond the issue's list: 16-byte accesses over several tiles (L a multiple of 4 above 1024); a hop below 32, whose tiles are 32
# hops; a look-back of more than one wavefront's 64 frames
EXTRA_MIX = [(3, 2, 2052, None, HOP), (3, 1, 2052, (2, 3, "above"), HOP), (3, 1, 700, (0, 5, "below"), 5), (2, 2, 700, (70, 30, "above"), 5)]


@functools.lru_cache(maxsize=None)
def mix_case(V, C, L, gate, hop=HOP):
    """-> dict: audio fp32 [B V, L], gain and pan (or None), the fp32 table, active bool [B V, T] or None, and the loops' fp64
    answer and magnitudes; computed once for the CPU and the device tests"""
    B = 2 if V < 64 else 1
    rng = np.random.default_rng(V * 1000 + C * 100 + L + (0 if gate is None else 7 + gate[0] + 2 * gate[1]))
    audio = rng.standard_normal((B * V, L)).astype(np.float32)
    gain = torch.from_numpy(rng.standard_normal((B, V)))
    pan = torch.from_numpy(rng.uniform(-1.0, 1.0, (B, V))) if C == 2 else None
    table = voices._gain_table(gain, pan, B, V, "cpu", "test").numpy()
    active, hold, fade = None, 0, 0
    if gate is not None:
        hold, fade, side = gate
        T = L // hop + 3 if side == "above" else max(L // hop - 1, 1)
        active = rng.random((B * V, T)) < (0.3 if hold < 64 else 0.01)
        active[B * V - 1] = False                                       # a row that is never active
        active[0] = False
        active[0, T - 1] = True                                         # a row active only in its last frame
    want, mag = vref.mix(audio.tolist(), table.tolist(), None if active is None else active.tolist(), V, hop, hold, fade)
    return dict(B=B, hop=hop, audio=audio, gain=gain, pan=pan, table=table, active=active, hold=hold, fade=fade,
                want=np.array(want), mag=np.array(mag))


def check_mix(got, case, V, what):
    got = got.reshape(case["want"].shape).astype(np.float64)
    bound = vref.roundings(V) * 2.0 ** -24 * case["mag"]
    err = np.abs(got - case["want"])
    worst = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print(what, "largest error over its bound:", round(worst, 4))
    assert bool((err <= bound).all()), (what, worst)


def run_mix(V, C, L, gate, device, hop=HOP):
    case = mix_case(V, C, L, gate, hop)
    active = None if case["active"] is None else torch.from_numpy(case["active"]).to(device)
    got = voices.mix_voices(torch.from_numpy(case["audio"]).to(device), V, gain=case["gain"], pan=case["pan"], active=active,
                            hop_length=None if active is None else hop, hold=case["hold"], fade=case["fade"])
    assert got.shape == ((case["B"], L) if C == 1 else (case["B"], 2, L)) and got.dtype == torch.float32
    check_mix(got.cpu().numpy(), case, V, (V, C, L, gate))
    if active is not None and V == 1:                                   # score B - 1 is the row that never plays
        assert bool((got[case["B"] - 1] == 0).all())
    return got


def check_ungated_single_voice_is_a_copy(device):
    x = torch.from_numpy(np.random.default_rng(3).standard_normal((5, 4 * 172 + 3)).astype(np.float32))
    x[0, :3] = torch.tensor([-0.0, float("inf"), 1e-42])
    got = voices.mix_voices(x.to(device), 1)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), x.numpy().view(np.uint32))


@pytest.mark.parametrize("V,C,L", MIX_SHAPES)
def test_mix_is_within_its_derived_bound(V, C, L):
    for gate in GATES:
        run_mix(V, C, L, gate, "cpu")


@pytest.mark.parametrize("V,C,L,gate,hop", EXTRA_MIX)
def test_mix_over_tiles_small_hops_and_long_look_backs(V, C, L, gate, hop):
    run_mix(V, C, L, gate, "cpu", hop)


def test_mix_of_one_voice_without_a_gate_copies_the_bits():
    check_ungated_single_voice_is_a_copy("cpu")


def test_the_gate_holds_fades_and_interpolates():
    """the envelope by hand: active in frame 1 only, hold 1, fade 2 -> e = 0, 1, 1, 1/2, 0, 0 and straight lines between"""
    active = torch.tensor([[0, 1, 0, 0, 0, 0]], dtype=torch.bool)
    got = voices.mix_voices(torch.ones(1, 6 * 4 + 3), 1, active=active[..., None], hop_length=4, hold=1, fade=2).numpy()[0]
    want = [0, .25, .5, .75] + [1] * 4 + [1, .875, .75, .625] + [.5, .375, .25, .125] + [0] * 11
    assert got.tolist() == want
    assert voices._envelope_host(active[0].numpy(), 1, 2).tolist() == [0, 2, 2, 1, 0, 0]
    assert voices._envelope_host(active[0].numpy(), 1, 0).tolist() == [0, 1, 1, 0, 0, 0]
    out = torch.full((1, 2, 27), 9.0)
    same = voices.mix_voices(torch.ones(1, 27), 1, pan=[0.0], out=out)
    assert same is out and np.allclose(out.numpy(), np.sqrt(0.5), rtol=1e-6)


# ------------------------------------------------------------------------------------------------------------------ MIDI
def test_a_chord_survives_a_polyphonic_midi_round_trip(tmp_path):
    chord = Notes(onset=[0, 0, 0, 20, 20], frames=[20, 20, 30, 10, 5], pitch=[60, 64, 67, 60, 76], level=[0.5, 0.25, 1.0, 0.75, 0.5])
    path = str(tmp_path / "chord.mid")
    chord.write_midi(path, 500, 48000, polyphonic=True)                 # (10 ticks a frame: exact)
    back = Notes.read_midi(path, 500, 48000, polyphonic=True)
    for k in ("onset", "frames", "pitch"):
        assert getattr(back, k).tolist() == getattr(chord, k).tolist(), k
    assert np.allclose(back.level.numpy(), chord.level.numpy(), atol=1.0 / 127) and back.scale == "chromatic"
    # the same pitch twice at once: a note-off closes the older note
    twice = Notes(onset=[0, 5], frames=[20, 30], pitch=[60, 60])
    twice.write_midi(path, 500, 48000, polyphonic=True)
    back = Notes.read_midi(path, 500, 48000, polyphonic=True)
    assert back.onset.tolist() == [[0, 5]] and back.frames.tolist() == [[20, 30]]
    # and the voices play it: three voices take the chords whole, the re-struck C in the voice that had it
    found, info = voices.allocate_voices(chord, 3, return_info=True)
    assert info["voice"].tolist() == [[0, 1, 2, 0, 1]] and int(info["stolen"]) == 0


def test_the_default_midi_calls_are_the_monophonic_ones(tmp_path):
    chord = Notes(onset=[0, 0, 10], frames=[20, 20, 5], pitch=[60, 64, 72], level=[1.0, 1.0, 0.0])
    a, b = str(tmp_path / "a.mid"), str(tmp_path / "b.mid")
    chord.write_midi(a, 500, 48000)
    chord.write_midi(b, 500, 48000, polyphonic=False)
    data = open(a, "rb").read()
    assert data == open(b, "rb").read()
    # by hand: 60 has no length (64 begins with it), 64 is cut at frame 10, 72 sounds 5 frames; 10 ticks a frame
    track = (b"\x00\xff\x51\x03\x07\xa1\x20" + b"\x00\x90\x40\x7f" + b"\x64\x80\x40\x00" + b"\x00\x90\x48\x01" + b"\x32\x80\x48\x00" +
             b"\x00\xff\x2f\x00")
    assert data == b"MThd" + struct.pack(">IHHH", 6, 0, 1, 480) + b"MTrk" + struct.pack(">I", len(track)) + track
    chord.write_midi(b, 500, 48000, polyphonic=True)
    mono, mono_again = Notes.read_midi(b, 500, 48000), Notes.read_midi(b, 500, 48000, polyphonic=False)
    # a note-on cuts the sounding note: 60 is cut at once, 64 at frame 10, 72 ends by its own note-off
    for notes in (mono, mono_again):
        assert notes.onset.tolist() == [[0, 10]] and notes.frames.tolist() == [[10, 5]] and notes.pitch.tolist() == [[64, 72]]
    assert Notes.read_midi(b, 500, 48000, polyphonic=True).pitch.tolist() == [[60, 64, 72]]


# ------------------------------------------------------------------------------------------------------------------ wiring
def test_entry_points_are_wired_and_validate_in_the_house_order():
    L = ddsp._lib.lib()
    assert L.ddsp_hip_abi_version() == 5 == ddsp._lib.ABI_VERSION
    names = list(ddsp._lib.SIGNATURES)
    at = names.index("ddsp_mfcc")
    assert names[at + 1:at + 3] == ["ddsp_voices_allocate", "ddsp_voices_mix"]
    header = open(os.path.join(ROOT, "include", "ddsp_hip.h")).read()
    assert header.index("int ddsp_mfcc(") < header.index("int ddsp_voices_allocate(") < header.index("int ddsp_voices_mix(") < \
        header.index("int ddsp_pcm_to_mono(")
    assert {"voices", "allocate_voices", "mix_voices"} <= set(ddsp.__all__) and ddsp.allocate_voices is voices.allocate_voices
    assert "ddsp_voices.hip" in open(os.path.join(ROOT, "ddsp-pytorch_amd", "csrc", "Makefile")).read()
    EINVAL, ERANGE, N = -1, -2, None
    word = ctypes.c_uint64(0)                                            # (a valid address; nothing is read from it)
    p = ctypes.addressof(word)
    alloc = lambda ptr, B, Ns, V, Nv, a=0, s=0, gap=0: L.ddsp_voices_allocate(*[ptr] * 16, B, Ns, V, Nv, a, s, gap, N)     # noqa: E731
    # options first, also with an empty batch; then the empty batch; then pointers, also with sizes out of range; then sizes
    for bad in (dict(V=0), dict(V=65), dict(a=3), dict(a=-1), dict(s=3), dict(gap=-1), dict(gap=1 << 24), dict(Ns=-1), dict(Nv=-1)):
        args = dict(dict(ptr=N, B=0, Ns=4, V=4, Nv=4), **bad)
        assert alloc(**args) == EINVAL, bad
    assert alloc(N, -1, 4, 4, 4) == EINVAL and alloc(N, 0, 4, 4, 4) == 0 and alloc(N, 0, 1 << 40, 64, 1 << 40) == 0
    assert alloc(N, 1, 4, 4, 4) == EINVAL and alloc(N, 1 << 20, 1 << 20, 4, 4) == EINVAL
    assert alloc(p, 1 << 20, 1 << 20, 4, 4) == ERANGE and alloc(p, 1 << 20, 4, 64, 1 << 10) == ERANGE
    mix = lambda ptr, B, V, C, Ls, T=0, hop=0, hold=0, fade=0, act=N: L.ddsp_voices_mix(ptr, ptr, act, ptr, B, V, C, Ls, T, hop, hold, fade, N)  # noqa: E731
    for bad in (dict(V=0), dict(V=65), dict(C=0), dict(C=3), dict(Ls=0), dict(hold=-1), dict(fade=-1), dict(hold=1 << 15, fade=1 << 15),
                dict(act=p, T=0, hop=64), dict(act=p, T=4, hop=0)):
        args = dict(dict(ptr=N, B=0, V=4, C=1, Ls=64), **bad)
        assert mix(**args) == EINVAL, bad
    assert mix(N, -1, 4, 1, 64) == EINVAL and mix(N, 0, 4, 1, 64) == 0 and mix(N, 0, 4, 2, 1 << 40) == 0
    assert mix(N, 1, 4, 1, 64) == EINVAL and mix(N, 1, 4, 1, 1 << 31) == EINVAL
    assert mix(p, 1, 4, 1, 1 << 31) == ERANGE and mix(p, 1 << 30, 4, 1, 1 << 20) == ERANGE
    assert mix(p, 1, 4, 1, 64, T=4, hop=(1 << 15) + 1, act=p) == ERANGE and mix(p, 1, 4, 1, 64, T=1 << 31, hop=64, act=p) == ERANGE


def test_python_refusals():
    notes = Notes(onset=[0, 0], frames=[5, 5], pitch=[60, 64])
    for bad in (dict(voices=0), dict(voices=65), dict(voices=2.0), dict(voices=True), dict(voices=2, assign="highest"),
                dict(voices=2, steal="loudest"), dict(voices=2, gap=-1), dict(voices=2, gap=1 << 24), dict(voices=2, max_notes=-1)):
        with pytest.raises(ValueError, match="allocate_voices"):
            voices.allocate_voices(notes, **bad)
    with pytest.raises(ValueError, match="allocate_voices"):
        voices.allocate_voices(dict(onset=[0]), 2)
    graded = Notes(onset=[0], frames=[5], pitch=[60])
    graded.level.requires_grad_(True)
    with pytest.raises(RuntimeError, match="allocate_voices"):
        voices.allocate_voices(graded, 2)
    x = torch.zeros(6, 100)
    on = torch.ones(6, 3, 1, dtype=torch.bool)
    for bad in (dict(voices=4), dict(voices=0), dict(voices=3, hold=-1), dict(voices=3, hold=1 << 15, fade=1 << 15), dict(voices=3, active=on),
                dict(voices=3, active=on, hop_length=0), dict(voices=3, active=on, hop_length=(1 << 15) + 1),
                dict(voices=3, active=on[:5], hop_length=64), dict(voices=3, active=on.float(), hop_length=64), dict(voices=3, gain=[1.0, 2.0]),
                dict(voices=3, pan=[0.0, 0.5, 1.5]), dict(voices=3, gain=[1.0, float("nan"), 1.0]), dict(voices=3, pan=torch.zeros(4, 3)),
                dict(voices=3, out=torch.zeros(2, 2, 100)), dict(voices=3, pan=[0.0] * 3, out=torch.zeros(2, 100))):
        with pytest.raises(ValueError, match="mix_voices"):
            voices.mix_voices(x, **bad)
    with pytest.raises(ValueError, match="mix_voices"):
        voices.mix_voices(torch.zeros(6), 3)
    with pytest.raises(RuntimeError, match="mix_voices"):
        voices.mix_voices(torch.zeros(6, 10, requires_grad=True), 3)
    ae_play = ddsp.AutoEncoder.play
    with pytest.raises(ValueError, match="voices=V"):
        ae_play(None, notes, frames=5, voice_options=dict(assign="lowest"))
