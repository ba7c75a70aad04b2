"""`note_expression`, `render_notes(..., expression=...)`, `Expression` and `Notes.sorted(return_order=True)` on CPU tensors
(the numpy path of ddsp_pytorch_amd/notes.py) against the plain loops of tests/notes_expression_reference.py, the properties that
follow from the definition, and the two entry points' argument checks.  The helpers take a device, and
tests/test_gpu_notes_expression.py runs them on the kernels.

Tolerances, section 10f's for the same reasons.  `bend`, `owner`, `position` (without synthetic vibrato) and the fill values are
held to the bit; normalized_cents to the bit against the definition evaluated in fp64 on the reference's position (with
synthetic vibrato: on the result's own position, which lies within 1 unit); f0 (through exp2) and loudness (an fp64 expression
that may be contracted before its one rounding to fp32) within 1 fp32 ulp.  A NaN loudness must be a NaN; its payload is not
part of the definition (inf - inf gives a NaN of either sign, depending on the machine)."""
import ctypes

import numpy as np
import pytest
import torch

import ddsp_pytorch_amd as ddsp
import notes_expression_reference as xref
import notes_reference as nref
import tuning_reference as ref
from ddsp_pytorch_amd.notes import Expression, Notes, _time_map_host, extract_notes, note_expression, render_notes
from test_host_abi import declared_prototypes
from test_notes_host import (HOP, RECORDS, RENDER_N, RENDER_OPTIONS, SR, designed_records, loop_options, make_records, notes_of, records_of)
from test_tuning_host import same_bits, within_one_ulp, z_of

NEW_SYMBOLS = ("ddsp_notes_expression", "ddsp_notes_render_expr")
SHAPES_T = [1, 63, 64, 65, 255, 256, 257, 513]                  # the render's tiles are 256 frames
# the expressive options: the defaults, kept ends shorter and longer than any note, amounts of either sign, no dynamics
EXPR_OPTIONS = [dict(), dict(keep_attack=2, keep_release=3), dict(keep_attack=1000), dict(keep_release=1000, bend_amount=0.5),
                dict(bend_amount=-1.75, dynamics_amount=0.3, keep_attack=1), dict(dynamics_amount=0.0, keep_release=1), dict(bend_amount=0.0)]


# ------------------------------------------------------------------------------------------------------------------ helpers
def make_source(seed, B, Tsrc, Nsrc, loudness=True, special=True):
    """A source that is no performance at all -- the render is defined for any: seeded records with onsets before 0 and past
    Tsrc, invalid lengths and NaN levels (make_records), a bend of up to +-300 cents, a loudness with NaN and +-inf in it."""
    rng = np.random.default_rng(seed)
    src = make_records(seed, B, Nsrc, Tsrc)
    src["bend"] = rng.integers(-300 * 65536, 300 * 65536, (B, Tsrc)).astype(np.int32)
    src["loudness"] = None
    if loudness:
        src["loudness"] = (rng.random((B, Tsrc)) * 4.0 - 3.0).astype(np.float32)
        if special:
            for value in (np.nan, np.inf, -np.inf):
                src["loudness"].reshape(-1)[rng.integers(0, B * Tsrc)] = value
    return src


def expression_of(src, device):
    return Expression(*(None if src[k] is None else torch.from_numpy(src[k]) for k in ("bend", "loudness", "onset", "frames", "level", "count"))).to(device)


def got_expr_render(notes, T, e, source=None, **options):
    source = None if source is None else torch.from_numpy(source).to(notes.device)
    z = render_notes(notes, T, SR, HOP, return_info=True, expression=e, source=source, **options)
    B = notes.rows
    for k in ("f0", "normalized_cents", "loudness", "harmonicity", "voiced"):
        assert z[k].shape == (B, T, 1) and z[k].dtype == (torch.bool if k == "voiced" else torch.float32), k
    out = {k: v.cpu().numpy().reshape(B, T) for k, v in z.items()}
    out["cents"] = out.pop("normalized_cents")
    return out


def close_levels(got, want):
    """fp32 arrays: a NaN where the other has one, elsewhere equal bits or finite neighbours"""
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan)) and within_one_ulp(np.where(nan, np.float32(0), got), np.where(nan, np.float32(0), want))


def check_expr_render(got, want, where, vibrato=False):
    assert same_bits(got["owner"], want["owner"]), (where, "owner")
    if vibrato:
        assert got["position"].dtype == np.int64 and np.abs(got["position"] - want["position"]).max() <= 1, (where, "position")
    else:
        assert same_bits(got["position"], want["position"]), (where, "position")
    cents, f0 = nref.controls_of(got["position"] if vibrato else want["position"])
    assert same_bits(got["cents"], cents), (where, "cents")
    assert within_one_ulp(got["f0"], f0), (where, "f0")
    assert close_levels(got["loudness"], want["loudness"]), (where, "loudness")
    assert same_bits(got["harmonicity"], want["harmonicity"]) and same_bits(got["voiced"], want["voiced"]), where


def split_options(options):
    """render_notes' options -> (the plain loops' render options, the expressive ones under the loops' names)"""
    o = dict(options)
    expr = dict(bend_amount=o.pop("bend_amount", 1.0), dyn_amount=o.pop("dynamics_amount", 1.0), keep_attack=o.pop("keep_attack", 0),
                keep_release=o.pop("keep_release", 0))
    return loop_options(o), expr


def run_expr_case(rec, offset, T, src, source, device, options, where):
    plain, expr = split_options(options)
    want = xref.render_expr(rec, offset, T, src, source=source, **plain, **expr)
    got = got_expr_render(notes_of(rec, offset, device), T, expression_of(src, device), source, **options)
    check_expr_render(got, want, (where, options), vibrato="vibrato_cents" in options)
    return want


def run_expression_cases(T, device):
    """note_expression on a seeded track: under the notes found on it, and under records that have nothing to do with it"""
    B = 3
    x = ref.make(400 + T, B, T, special=True)
    z = z_of(x, device, keys=("cents", "f0", "loud"))
    found = extract_notes(z, min_note_frames=2 if T > 4 else 0)
    cases = [(found, records_of(found), found.offset.cpu().numpy())]
    for N in RENDER_N:
        rec = make_records(410 + T + N, B, N, T)
        offset = [(-50, 0, 37)[(b + N) % 3] for b in range(B)] if N % 2 else [13]          # G = B and G = 1
        cases.append((notes_of(rec, offset, device), rec, offset))
    for notes, rec, offset in cases:
        want = xref.expression(x["cents"], rec, offset)
        e = note_expression(z, notes, return_owner=True)
        assert e.device.type == device and e.bend.dtype == torch.int32 and e.owner.dtype == torch.int32 and e.bend.shape == (B, T)
        assert same_bits(e.bend.cpu().numpy(), want["bend"]) and same_bits(e.owner.cpu().numpy(), want["owner"]), (T, rec["onset"].shape)
        assert note_expression(z, notes).owner is None and same_bits(e.loudness.cpu().numpy(), x["loud"])
        for k in ("onset", "frames", "level", "count"):
            assert same_bits(getattr(e, k).cpu().numpy(), rec[k]), k
    if T >= 63:
        assert (want["owner"] >= 0).any() and (want["owner"] < 0).any() and want["bend"].any()


def run_expr_render_cases(T, device):
    """every N at this T, against two source lengths: across the parameters every T meets every tile path of Tsrc as well"""
    at = SHAPES_T.index(T)
    for j, N in enumerate(RENDER_N):
        for Tsrc in (SHAPES_T[(at + 3 + j) % 8], SHAPES_T[(2 * at + j) % 8]):
            B = 3 if N < 300 else 2
            Nsrc = RENDER_N[(j + at) % 5]
            rec = make_records(500 + T + N, B, N, T)
            src = make_source(600 + Tsrc + Nsrc, B, Tsrc, Nsrc, loudness=(at + j) % 3 != 0)
            rng = np.random.default_rng(T + N)
            source = None if (at + j) % 2 else rng.integers(-3, Nsrc + 3, (B, N)).astype(np.int32)
            offset = [(-50, 0, 37)[(b + N) % 3] for b in range(B)] if N % 2 else [13]
            for i in range(2):
                options = dict(RENDER_OPTIONS[(3 * j + T + 5 * i) % len(RENDER_OPTIONS)], **EXPR_OPTIONS[(at + j + 3 * i) % len(EXPR_OPTIONS)])
                run_expr_case(rec, offset, T, src, source, device, options, (T, N, Tsrc, Nsrc))


@pytest.mark.parametrize("T", SHAPES_T)
def test_cpu_expression_equals_plain_loops(T):
    run_expression_cases(T, "cpu")


@pytest.mark.parametrize("T", SHAPES_T)
def test_cpu_expressive_render_equals_plain_loops(T):
    run_expr_render_cases(T, "cpu")


# ------------------------------------------------------------------------------------------------------------------ properties
def check_no_expression_is_no_change(device):
    """expression=None is the plain call; a zero bend without loudness, and a source of -1 everywhere, give its bits"""
    T = 44
    rec = designed_records(T)
    B, N = rec["onset"].shape
    notes = notes_of(rec, [21], device)
    src = make_source(700, B, 50, N, special=False)
    for k in ("onset", "frames", "level", "count"):
        src[k] = rec[k]
    zero = dict(src, bend=np.zeros_like(src["bend"]), loudness=None)
    none = np.full((B, N), -1, np.int32)
    for options in RENDER_OPTIONS:
        plain = render_notes(notes, T, SR, HOP, return_info=True, **options)
        again = render_notes(notes, T, SR, HOP, return_info=True, expression=None, **options)
        silent = render_notes(notes, T, SR, HOP, return_info=True, expression=expression_of(zero, device), **options)
        nowhere = render_notes(notes, T, SR, HOP, return_info=True, expression=expression_of(src, device), source=torch.from_numpy(none).to(device),
                               **options)
        for k in plain:
            for other in (again, silent, nowhere):
                assert same_bits(plain[k].cpu().numpy(), other[k].cpu().numpy()), (options, k)
        moved = render_notes(notes, T, SR, HOP, return_info=True, expression=expression_of(src, device), **options)
        assert not torch.equal(moved["position"], plain["position"])            # (and the same source, read, does change it)


def test_no_expression_is_no_change():
    check_no_expression_is_no_change("cpu")


def vibrato_melody():
    """section 10e's melody with a 5.5 Hz, +-30 cent vibrato added; a loudness on a grid of 2^-10 in [0, 1]"""
    cents, _ = ref.melody()
    t = np.arange(cents.shape[1])
    c = 7180.0 * cents.astype(np.float64) + ref.K + 30.0 * np.sin(2.0 * np.pi * 5.5 * HOP / SR * t)[None]
    n = ((c - ref.K) / 7180.0).astype(np.float32)
    loud = (np.random.default_rng(8).integers(0, 1025, n.shape) / 1024.0).astype(np.float32)
    return dict(cents=n, f0=ref.f0_of_cents(n), loud=loud)


def positions_of(cents):
    return np.array([[ref.position(v) for v in row] for row in cents], dtype=np.int64)


def check_round_trip(device):
    x = vibrato_melody()
    T = x["cents"].shape[1]
    z = z_of(x, device, keys=("cents", "f0", "loud"))
    notes = extract_notes(z, min_note_frames=3)
    e = note_expression(z, notes, return_owner=True)
    out = render_notes(notes, T, SR, HOP, floor=0.0, expression=e, return_info=True)
    owner = out["owner"].cpu().numpy()
    kept = owner >= 0
    assert same_bits(owner, e.owner.cpu().numpy()) and kept.mean() > 0.8 and int(notes.count[0]) > 10
    u = positions_of(x["cents"])
    assert np.array_equal(out["position"].cpu().numpy()[kept], u[kept])         # to the bit
    got = out["normalized_cents"].cpu().numpy().reshape(1, T)
    assert within_one_ulp(got[kept], x["cents"][kept])
    assert same_bits(out["loudness"].cpu().numpy().reshape(1, T)[kept], x["loud"][kept])
    assert np.abs(e.bend.cpu().numpy()).max() > 20 * 65536                      # there is a curve to lose


def test_round_trip():
    check_round_trip("cpu")


def check_edits_carry_the_curve(device):
    """transposed by 3 semitones and moved 7 frames later, every note still wears its source's bend, frame for frame"""
    x = vibrato_melody()
    T = x["cents"].shape[1]
    z = z_of(x, device, keys=("cents", "f0", "loud"))
    notes = extract_notes(z, min_note_frames=3)
    e = note_expression(z, notes)
    edited = notes.transpose(3)._with(onset=torch.where(notes._used(), notes.onset + 7, notes.onset))
    out = render_notes(edited, T + 7, SR, HOP, expression=e, return_info=True)
    position, owner = out["position"].cpu().numpy()[0], out["owner"].cpu().numpy()[0]
    rec, bend, o = records_of(notes), e.bend.cpu().numpy()[0], int(notes.offset[0])
    n = int(rec["count"][0])
    for i in range(n):
        s, L = int(rec["onset"][0, i]), int(rec["frames"][0, i])
        centre = (int(rec["pitch"][0, i]) + 3) * ref.S + int(rec["detune"][0, i]) + 65536 * o
        assert (owner[s + 7:s + 7 + L] == i).all() and np.array_equal(position[s + 7:s + 7 + L] - centre, bend[s:s + L]), i
    assert n > 10


def test_edits_carry_the_curve():
    check_edits_carry_the_curve("cpu")


def check_stretched_ramp(device):
    """a note whose bend is the ramp 1000 k, played twice as long: every frame within 1 unit of 1000 (its position in source
    frames); with kept ends the head and the tail are the source's own frames"""
    Ls = 37
    src = dict(onset=np.array([[5]], np.int32), frames=np.array([[Ls]], np.int32), level=np.array([[0.5]], np.float32),
               count=np.array([1], np.int32), bend=np.zeros((1, 60), np.int32), loudness=None)
    src["bend"][0, 5:5 + Ls] = 1000 * np.arange(Ls)
    notes = Notes(onset=[3], frames=[2 * Ls], pitch=[60]).to(device)
    for keep_attack, keep_release in ((0, 0), (4, 6)):
        out = render_notes(notes, 90, SR, HOP, expression=expression_of(src, device), keep_attack=keep_attack, keep_release=keep_release,
                           return_info=True)
        got = out["position"].cpu().numpy()[0, 3:3 + 2 * Ls] - 60 * ref.S
        for k in range(2 * Ls):
            q, f = xref.time_map(Ls, 2 * Ls, keep_attack, keep_release, k)
            assert abs(int(got[k]) - 1000 * (q + f / 65536.0)) <= 1, (k, got[k], q, f)
        assert np.array_equal(got[:keep_attack], 1000 * np.arange(keep_attack))
        assert np.array_equal(got[2 * Ls - keep_release:], 1000 * np.arange(Ls - keep_release, Ls))
        assert (np.diff(got) >= 0).all() and got[-1] == 1000 * (Ls - 1)


def test_a_stretched_ramp():
    check_stretched_ramp("cpu")


def check_amounts(device):
    B, N, T, Tsrc = 2, 30, 172, 200
    rec = make_records(720, B, N, T)
    rec["count"][:] = N
    src = make_source(721, B, Tsrc, N, special=False)
    notes, e = notes_of(rec, [5], device), expression_of(src, device)
    options = dict(attack=2, release=3, floor=-2.0, keep_attack=1)
    render = lambda **kw: {k: v.cpu().numpy().reshape(B, T) for k, v in                                      # noqa: E731
                           render_notes(notes, T, SR, HOP, return_info=True, **options, **kw).items()}
    plain = render_notes(notes, T, SR, HOP, return_info=True, attack=2, release=3, floor=-2.0)
    plain = {k: v.cpu().numpy().reshape(B, T) for k, v in plain.items()}
    full, none, half, still = render(expression=e), render(expression=e, bend_amount=0.0), render(expression=e, bend_amount=0.5), \
        render(expression=e, dynamics_amount=0.0)
    assert same_bits(none["position"], plain["position"]) and same_bits(none["normalized_cents"], plain["normalized_cents"])
    assert same_bits(still["loudness"], plain["loudness"]) and same_bits(still["position"], full["position"])
    bend = full["position"] - plain["position"]                                # amount 1 is exact: B itself
    assert np.array_equal(half["position"] - plain["position"], np.rint(0.5 * bend.astype(np.float64)).astype(np.int64))
    assert (bend != 0).any() and (bend % 2 != 0).any() and not same_bits(full["loudness"], plain["loudness"])
    assert same_bits(none["loudness"], full["loudness"])


def test_amounts():
    check_amounts("cpu")


# the tiles are 256 frames: notes across one and two tile boundaries, a note in a tile's last frame and in its first
TILE_NOTES = [[(10, 100, 60), (200, 380, 64), (590, 10, 67)], [(100, 155, 60), (255, 1, 62), (256, 1, 64), (257, 100, 65), (500, 30, 67)]]
TILE_SOURCE = [[(0, 50, 60), (250, 263, 64), (513, 4, 67)], [(0, 255, 60), (255, 1, 62), (256, 1, 64), (300, 40, 65), (505, 8, 67)]]


def tile_case():
    T, Tsrc = 600, 517
    rec = dict(onset=np.zeros((2, 5), np.int32), frames=np.zeros((2, 5), np.int32), pitch=np.zeros((2, 5), np.int32), detune=np.zeros((2, 5), np.int32),
               level=np.full((2, 5), 0.25, np.float32), count=np.array([3, 5], np.int32))
    src = make_source(730, 2, Tsrc, 5, special=False)
    for b in range(2):
        for i, ((s, L, p), (so, Ls, _)) in enumerate(zip(TILE_NOTES[b], TILE_SOURCE[b])):
            rec["onset"][b, i], rec["frames"][b, i], rec["pitch"][b, i] = s, L, p
            src["onset"][b, i], src["frames"][b, i], src["level"][b, i] = so, Ls, 0.5
    src["count"] = np.array([3, 5], np.int32)
    return rec, src, T


def check_tile_boundaries(device):
    rec, src, T = tile_case()
    for options in (dict(), dict(keep_attack=3, keep_release=2, glide=4, release=5)):
        want = run_expr_case(rec, [0], T, src, None, device, options, "tiles")
        assert (want["owner"][1, 255:258] == [1, 2, 3]).all() and (want["owner"][0, 200:580] == 1).all()
    # and the expression of a track under those notes
    x = ref.make(731, 2, T)
    z = z_of(x, device, keys=("cents", "f0"))
    want = xref.expression(x["cents"], rec, [0])
    e = note_expression(z, notes_of(rec, [0], device), return_owner=True)
    assert same_bits(e.bend.cpu().numpy(), want["bend"]) and same_bits(e.owner.cpu().numpy(), want["owner"])


def test_notes_at_the_tile_boundaries():
    check_tile_boundaries("cpu")


def crowded_case():
    """400 notes on 40 frames: more records than a tile stages, so they are read from global memory"""
    rec = make_records(740, 2, 400, 40)
    rec["count"][:] = 400
    src = make_source(741, 2, 65, 64)
    source = np.random.default_rng(742).integers(-1, 66, (2, 400)).astype(np.int32)
    return rec, src, source


def test_a_crowded_row():
    rec, src, source = crowded_case()
    run_expr_case(rec, [5], 40, src, source, "cpu", dict(glide=4, keep_attack=1), "crowded")


def test_time_map():
    sizes = (1, 2, 3, 5, 64, 65)
    cases = [(a, b, c, d) for a in sizes for b in sizes for c in sizes for d in sizes] + [((1 << 24) - 1, 3, 0, 0)]
    for Ls, Lp, ka, kr in cases:
        a = min(ka, Ls, Lp)
        r = min(kr, Ls - a, Lp - a)
        got = [xref.time_map(Ls, Lp, ka, kr, k) for k in range(Lp)]
        assert all(0 <= q <= Ls - 1 and 0 <= f < 65536 and (f == 0 or q < Ls - 1) for q, f in got), (Ls, Lp, ka, kr)
        assert all(x <= y for x, y in zip(got, got[1:])), (Ls, Lp, ka, kr)      # (q, f) in order: non-decreasing in k
        if Lp == Ls:
            assert got == [(k, 0) for k in range(Lp)], (Ls, Lp, ka, kr)
        assert got[:a] == [(k, 0) for k in range(a)] and got[Lp - r:] == [(Ls - r + k, 0) for k in range(r)], (Ls, Lp, ka, kr)
        k = np.arange(Lp, dtype=np.int64)
        q, f = _time_map_host(k, np.full_like(k, Lp), np.full_like(k, Ls), ka, kr)
        assert q.dtype == np.int64 and list(zip(q.tolist(), f.tolist())) == got, (Ls, Lp, ka, kr)
    # the longest note there is: every frame through the vectorised form, which the sampled frames hold to the Python integers
    Ls, Lp, ka, kr = 3, (1 << 24) - 1, 1, 1
    k = np.arange(Lp, dtype=np.int64)
    q, f = _time_map_host(k, np.full_like(k, Lp), np.full_like(k, Ls), ka, kr)
    rng = np.random.default_rng(3)
    for at in list(range(2000)) + list(range(Lp - 2000, Lp)) + rng.integers(0, Lp, 20000).tolist() + [Lp // 2 - 1, Lp // 2, Lp // 2 + 1]:
        assert (int(q[at]), int(f[at])) == xref.time_map(Ls, Lp, ka, kr, at), at
    whole = q * 65536 + f
    assert (np.diff(whole) >= 0).all() and q.min() == 0 and q.max() == Ls - 1 and (f[q == Ls - 1] == 0).all()
    assert (int(q[0]), int(f[0])) == (0, 0) and (int(q[-1]), int(f[-1])) == (Ls - 1, 0)


# ------------------------------------------------------------------------------------------------------------------ the objects
def test_expression_object_sorted_order_and_errors():
    x = ref.make(750, 2, 40)
    z = z_of(x, keys=("cents", "f0", "loud"))
    notes = extract_notes(z)
    e = note_expression(z, notes, return_owner=True)
    assert (e.rows, e.source_frames, e.max_notes) == (2, 40, notes.max_notes) and e.device.type == "cpu"
    e.loudness[0, 0] = 99.0                                     # a copy: the source's track is not touched
    assert float(z["loudness"][0, 0, 0]) != 99.0
    back = Expression.from_dict(e.to_dict()).to("cpu")
    for k in ("bend", "loudness", "onset", "frames", "level", "count", "owner"):
        assert same_bits(getattr(back, k).numpy(), getattr(e, k).numpy()), k
    bare = note_expression(dict(normalized_cents=z["normalized_cents"]), notes)
    assert bare.loudness is None and bare.owner is None and Expression.from_dict(bare.to_dict()).loudness is None
    assert same_bits(bare.bend.numpy(), e.bend.numpy())
    # sorted(return_order=True): a re-ordered list still names its sources
    mixed = Notes(onset=[[9, 3, 3, 1, 50]], frames=[[1, 2, 3, 4, 5]], pitch=[[60, 61, 62, 63, 64]], count=[4])
    s, order = mixed.sorted(return_order=True)
    assert order.dtype == torch.int32 and order.tolist() == [[3, 1, 2, 0, 4]] and s.onset.tolist() == [[1, 3, 3, 9, 50]]
    assert same_bits(mixed.sorted().onset.numpy(), s.onset.numpy())
    src = make_source(751, 1, 30, 5, special=False)
    src["onset"], src["frames"], src["count"] = np.array([[20, 3, 9, 0, 25]], np.int32), np.array([[4, 5, 3, 3, 2]], np.int32), np.array([5], np.int32)
    ex = expression_of(src, "cpu")
    direct = render_notes(mixed.sorted(), 60, SR, HOP, expression=ex, source=order, return_info=True)
    want = xref.render_expr(records_of(s), [0], 60, src, source=order.numpy())
    assert same_bits(direct["position"].numpy(), want["position"]) and (want["position"] != nref.render(records_of(s), [0], 60)["position"]).any()
    n = Notes(onset=[0, 10], frames=[10, 8], pitch=[60, 62])
    one = Expression(np.zeros((1, 20), np.int32), None, n.onset, n.frames, n.level, n.count)
    args = dict(frames=20, sample_rate=SR, hop_length=HOP, expression=one)
    for bad in (dict(expression=3), dict(expression=Expression(np.zeros((2, 20), np.int32), None, [[0], [0]], [[1], [1]], [[0.0], [0.0]], [1, 1])),
                dict(source=[[0]]), dict(source=[[0, 1]], expression=None), dict(bend_amount=float("nan")), dict(bend_amount=16.5),
                dict(dynamics_amount=float("inf")), dict(dynamics_amount=-17.0), dict(keep_attack=-1), dict(keep_release=1 << 24), dict(keep_attack=1.5)):
        with pytest.raises(ValueError):
            render_notes(n, **dict(args, **bad))
    render_notes(n, **dict(args, source=[[1, 0]], bend_amount=-16.0, dynamics_amount=16.0, keep_attack=(1 << 24) - 1))
    for bad in (dict(bend=np.zeros((20,), np.int32)), dict(loudness=np.zeros((1, 19), np.float32)), dict(frames=[[1]]), dict(count=[1, 2]),
                dict(owner=np.zeros((2, 20), np.int32))):
        with pytest.raises(ValueError):
            Expression(**dict(dict(bend=np.zeros((1, 20), np.int32), loudness=None, onset=n.onset, frames=n.frames, level=n.level, count=n.count), **bad))
    with pytest.raises(ValueError):
        note_expression(z, n)                                   # one row of notes, two of controls
    with pytest.raises(ValueError):
        note_expression(z, 3)
    with pytest.raises(Exception, match="grad"):
        note_expression(dict(z, loudness=z["loudness"].clone().requires_grad_()), notes)
    assert hasattr(ddsp.AutoEncoder, "transcribe") and hasattr(ddsp.AutoEncoder, "play")


# ------------------------------------------------------------------------------------------------------------------ wiring, ABI
def test_symbols_and_entry_point_validation():
    names = list(declared_prototypes())
    L = ctypes.CDLL(ddsp._lib.SO_PATH)
    for name in NEW_SYMBOLS:
        assert name in ddsp._lib.EXPORTS and name in ddsp._lib.SIGNATURES and hasattr(L, name), name
    # tests/test_notes_host.py pins the table's last four entries, so the two sit in front of them
    at = names.index("ddsp_wfft_probe")
    around = ("ddsp_wfft_probe",) + NEW_SYMBOLS + ("ddsp_griffinlim_stage",)
    assert tuple(names[at:at + 4]) == around == tuple(ddsp._lib.SIGNATURES)[at:at + 4] == ddsp._lib.EXPORTS[at:at + 4]
    assert names[-1] == "ddsp_gather_batch" and ddsp._lib.ABI_VERSION == 5 == ddsp._lib.lib().ddsp_hip_abi_version()
    assert ddsp.Expression is Expression and ddsp.note_expression is note_expression
    assert {"Expression", "note_expression"} <= set(ddsp.__all__) and ddsp.notes.MAX_AMOUNT == 16.0
    L = ddsp._lib.lib()
    EINVAL, ERANGE = -1, -2
    word = (ctypes.c_uint64 * 8)()
    p = ctypes.addressof(word)

    def expression(B=1, T=5, N=3, groups=1, cents=p, onset=p, count=p, offset=p, bend=p, owner=None):
        return L.ddsp_notes_expression(cents, onset, p, p, p, count, offset, bend, owner, B, T, N, groups, None)

    assert expression(B=0) == 0 and expression(B=-1) == EINVAL and expression(T=0) == EINVAL and expression(N=-1) == EINVAL
    assert expression(B=0, cents=None, bend=None) == 0 and expression(B=-1, T=1 << 24) == EINVAL          # options, then the empty batch
    assert expression(cents=None) == EINVAL and expression(onset=None) == EINVAL and expression(count=None) == EINVAL
    assert expression(offset=None) == EINVAL and expression(bend=None) == EINVAL and expression(B=3, groups=2) == EINVAL
    assert expression(cents=None, T=1 << 24) == EINVAL                                                      # pointers before sizes
    assert expression(T=1 << 24) == ERANGE and expression(B=1 << 12, T=1 << 19, N=0) == ERANGE and expression(B=1 << 12, T=5, N=1 << 19) == ERANGE

    def render(B=1, T=5, N=3, groups=1, flags=1, transpose=0, glide=0, attack=0, release=0, delay=0, ramp=1, depth=0.0, omega=0.0, floor=0.0,
               default=1.0, onset=p, count=p, f0=p, voiced=p, source=None, src_onset=p, src_level=p, src_count=p, bend=p, loud=None, Tsrc=7, Nsrc=2,
               bend_amount=1.0, dyn_amount=1.0, keep_attack=0, keep_release=0):
        return L.ddsp_notes_render_expr(onset, p, p, p, p, count, p, f0, p, p, p, voiced, None, None, B, T, N, groups, flags, transpose, glide,
                                        attack, release, delay, ramp, depth, omega, floor, default, source, src_onset, p, src_level, src_count,
                                        bend, loud, Tsrc, Nsrc, bend_amount, dyn_amount, keep_attack, keep_release, None)

    # the render's own checks, in its order
    assert render(B=0) == 0 and render(B=-1) == EINVAL and render(T=0) == EINVAL and render(N=-1) == EINVAL and render(flags=4) == EINVAL
    assert render(transpose=128 * ref.S + 1) == EINVAL and render(glide=-1) == EINVAL and render(attack=1 << 24) == EINVAL
    assert render(release=-1) == EINVAL and render(delay=-1) == EINVAL and render(ramp=0) == EINVAL and render(depth=-1.0) == EINVAL
    assert render(omega=float("nan")) == EINVAL and render(floor=float("nan")) == EINVAL and render(default=float("inf")) == EINVAL
    # the new options
    assert render(Tsrc=0) == EINVAL and render(Nsrc=-1) == EINVAL and render(bend_amount=float("nan")) == EINVAL
    assert render(bend_amount=16.5) == EINVAL and render(dyn_amount=float("-inf")) == EINVAL and render(dyn_amount=-16.5) == EINVAL
    assert render(keep_attack=-1) == EINVAL and render(keep_attack=1 << 24) == EINVAL and render(keep_release=-1) == EINVAL
    assert render(keep_release=1 << 40) == EINVAL and render(bend_amount=16.0, dyn_amount=-16.0, keep_attack=(1 << 24) - 1, B=0) == 0
    # options before the empty batch, the empty batch before the pointers, the pointers before the sizes
    assert render(B=0, keep_attack=-1) == EINVAL and render(B=0, bend=None, f0=None) == 0
    assert render(onset=None) == EINVAL and render(count=None) == EINVAL and render(f0=None) == EINVAL and render(voiced=None) == EINVAL
    assert render(B=3, groups=2) == EINVAL and render(src_count=None) == EINVAL and render(bend=None) == EINVAL
    assert render(src_onset=None) == EINVAL and render(src_level=None) == EINVAL and render(src_onset=None, src_level=None, Nsrc=0, B=0) == 0
    assert render(bend=None, Tsrc=1 << 24) == EINVAL and render(f0=None, T=1 << 24) == EINVAL
    assert render(T=1 << 24) == ERANGE and render(B=1 << 12, T=1 << 19, N=0) == ERANGE and render(B=1 << 12, T=5, N=1 << 19) == ERANGE
    assert render(Tsrc=1 << 24) == ERANGE and render(B=1 << 12, Tsrc=1 << 19) == ERANGE and render(B=1 << 12, Nsrc=1 << 19) == ERANGE
