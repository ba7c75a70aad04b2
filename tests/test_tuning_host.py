"""`tuning_statistics` and `tune_pitch` on CPU tensors (the numpy path of ddsp_pytorch_amd/tuning.py) against the plain-loop
definition of tests/tuning_reference.py, the properties that follow from the definition, and the ABI's additions.

Tolerances: none but one.  A position carries one fp64 rounding, and everything after it is integer arithmetic, so the
histogram, offset, root, profile, notes, correction and normalized_cents agree to the bit; f0 is formed through exp2 and is
compared within 1 fp32 ulp (the precedent of the voicing tests).  The helpers take a device, and tests/test_gpu_tuning.py runs
them on the kernels.

The hard-snap bound: a snapped frame's normalized_cents is n' = fl32(n + a), a = fl32(d / (65536 7180));
the two roundings are within ulp(n') / 2 and ulp(a) / 2, each worth 7180 cents per unit, and d was formed from a position
rounded to 2^-16 cent, within 2^-17: |7180 n' + K - (100 note + o)| <= 7180 (ulp(n') + ulp(a)) / 2 + 2^-17 cents.  Measured on
the plain loops (seed 41, 5 x 172): worst 2.18e-4 cents against a bound of 2.25e-4 there; no frame uses more than 0.983 of
its bound."""
import ctypes
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import ddsp_pytorch_amd as ddsp
import tuning_reference as ref
from ddsp_pytorch_amd.tuning import TuningStatistics, tune_pitch, tuning_statistics
from test_host_abi import declared_prototypes

NEW_SYMBOLS = ("ddsp_tuning_accum_bytes", "ddsp_tuning_stats", "ddsp_tuning_estimate", "ddsp_tuning_workspace_bytes",
               "ddsp_tuning_apply")
SHAPES = [(1, 1), (1, 2), (3, 5), (2, 63), (2, 64), (2, 65), (5, 172)]
# every option on and off; glide 0, 1, 4 and beyond T; min_note_frames 0 and 3; hysteresis 0 and 20; a per-row amount
OPTIONS = [dict(), dict(hysteresis=0.0), dict(vibrato=False), dict(concert=True), dict(vibrato=False, concert=True, hysteresis=0.0),
           dict(min_note_frames=3), dict(min_note_frames=3, vibrato=False, glide=1), dict(glide=1), dict(glide=4, hysteresis=0.0),
           dict(glide=10 ** 6), dict(glide=4, min_note_frames=3, concert=True), dict(amount=0.5),
           dict(amount="rows", glide=1, vibrato=False), dict(amount="rows", min_note_frames=3, hysteresis=0.0)]
GATES = [dict(), dict(voiced=True, silence=-3.0, confidence=0.2)]
KEYS = {"cents": "normalized_cents", "f0": "f0", "harm": "harmonicity", "loud": "loudness"}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def within_one_ulp(a, b):
    """fp32 arrays: equal bits, or finite neighbours"""
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    return bool(np.all((ia == ib) | ((np.abs(ia - ib) <= 1) & np.isfinite(a) & np.isfinite(b))))


def z_of(x, device="cpu", voiced=False, keys=("cents", "f0", "harm", "loud")):
    z = {KEYS[k]: torch.from_numpy(x[k])[..., None].to(device) for k in keys}
    if voiced:
        z["voiced"] = torch.from_numpy(x["voiced"])[..., None].to(device)
    return z


def on_of(x, gate):
    return ref.on_mask(x["cents"], x["harm"], x["loud"] if gate.get("silence") is not None else None,
                       x["voiced"] if gate.get("voiced") else None, gate.get("silence"), gate.get("confidence", 0.0))


def got_stats(x, device, gate, **kw):
    stats, hist = tuning_statistics(z_of(x, device, gate.get("voiced", False)), return_histogram=True, silence=gate.get("silence"),
                                    confidence=gate.get("confidence", 0.0), **kw)
    assert stats.device.type == device and hist.dtype == torch.int64
    return stats, dict(histogram=hist.cpu().numpy(), offset=stats.offset.cpu().numpy(), root=stats.root.cpu().numpy(),
                       profile=stats.profile.cpu().numpy(), frames=stats.frames.cpu().numpy())


def check_stats(got, want, where):
    for k in ("histogram", "offset", "root", "profile", "frames"):
        assert same_bits(got[k], want[k]), (where, k, got[k], want[k])


def got_tune(x, device, stats, gate, **options):
    options = dict(options)
    if isinstance(options.get("amount"), np.ndarray):
        options["amount"] = torch.from_numpy(options["amount"]).to(device)
    new, info = tune_pitch(z_of(x, device, gate.get("voiced", False)), stats, return_info=True, **options)
    return dict(notes=info["notes"].cpu().numpy(), correction=info["correction"].cpu().numpy(),
                cents=new["normalized_cents"].cpu().numpy()[..., 0], f0=new["f0"].cpu().numpy()[..., 0])


def check_tune(got, want, where):
    for k in ("notes", "correction", "cents"):
        assert same_bits(got[k], want[k]), (where, k)
    assert within_one_ulp(got["f0"], want["f0"]), (where, "f0")


def reference_options(options, B, seed=0):
    """tune_pitch's options -> (the call's, the reference's)"""
    call, loops = dict(options), dict(options)
    if options.get("amount") == "rows":
        rows = np.random.default_rng(seed).random(B).astype(np.float32)
        rows[0] = 1.0
        call["amount"], loops["amount"] = rows, rows
    loops["h"] = round(float(loops.pop("hysteresis", 20.0)) * 65536.0)
    return call, loops


def run_cases(R, T, device):
    for seed, low in ((40 + R, False), (50 + T, True)):
        x = ref.make(seed, R, T, special=True, low=low)
        for gate in GATES:
            on = on_of(x, gate)
            for per_row, scale, root in ((True, "major", None), (False, "major", None), (True, "pentatonic", None), (False, 0x5AD, 7)):
                mask = ref.SCALES.get(scale, scale)
                want = ref.statistics(x["cents"], on, per_row=per_row, mask=mask, root=root)
                stats, got = got_stats(x, device, gate, per_row=per_row, scale=scale, root=root)
                check_stats(got, want, (R, T, low, gate, per_row, scale))
                if (scale, per_row) == ("pentatonic", True) or (low and not per_row):
                    continue
                for options in OPTIONS if scale == "major" else OPTIONS[:3]:
                    call, loops = reference_options(options, R, seed)
                    exp = ref.tune(x["cents"], x["f0"], on, want["offset"], want["root"], mask, **loops)
                    check_tune(got_tune(x, device, stats, gate, **call), exp, (R, T, low, gate, per_row, scale, options))


@pytest.mark.parametrize("R,T", SHAPES)
def test_cpu_path_equals_plain_loops(R, T):
    run_cases(R, T, "cpu")


def check_measures_itself(device):
    """tuning=None: each row measured by itself, with the scale and root asked for"""
    x = ref.make(61, 3, 65, special=True)
    on = on_of(x, {})
    for scale, root in (("major", None), ("minor", 4)):
        own = ref.statistics(x["cents"], on, per_row=True, mask=ref.SCALES[scale], root=root)
        new, info = tune_pitch(z_of(x, device), scale=scale, root=root, return_info=True)
        exp = ref.tune(x["cents"], x["f0"], on, own["offset"], own["root"], ref.SCALES[scale], h=round(20 * 65536))
        assert same_bits(info["notes"].cpu().numpy(), exp["notes"]) and same_bits(info["offset"].cpu().numpy(), own["offset"])
        assert same_bits(info["root"].cpu().numpy(), own["root"])
        assert same_bits(new["normalized_cents"].cpu().numpy()[..., 0], exp["cents"])
        assert torch.equal(info["correction_cents"], info["correction"].double() / 65536.0)
    z = z_of(x, device)
    z["extra"] = object()
    out = tune_pitch(z)
    assert out["extra"] is z["extra"] and out["harmonicity"] is z["harmonicity"] and out["f0"] is not z["f0"] and list(out) == list(z)


def test_tuning_none_measures_each_row():
    check_measures_itself("cpu")


def find_cents(target):
    """an fp32 normalized_cents whose position is exactly `target` units, or None"""
    n0 = np.float32((target / 65536.0 - ref.K) / 7180.0)
    n = n0
    for _ in range(40):
        n = np.nextafter(n, np.float32(-np.inf))
    for _ in range(80):
        if ref.position(n) == target:
            return n
        n = np.nextafter(n, np.float32(np.inf))
    return None


def row_of(values):
    cents = np.array([values], dtype=np.float32)
    return dict(cents=cents, f0=ref.f0_of_cents(cents))


def check_designed_ties(device):
    # a frame exactly halfway between two allowed notes goes to the lower one: C major around note 60; 61 S lies halfway
    # between C (60) and D (62), 64.5 S between E (64) and F (65).  The offset is free, so some o puts a position there.
    found = 0
    for half, lower in ((61 * ref.S, 60), (64 * ref.S + ref.S // 2, 64), (63 * ref.S, 62)):
        for o in range(-50, 50):
            n = find_cents(half + 65536 * o)
            if n is None:
                continue
            x = row_of([n])
            stats = TuningStatistics(offset=o, root=0, scale="major").to(device)
            _, info = tune_pitch(z_of(x, device, keys=("cents", "f0")), stats, hysteresis=0.0, return_info=True)
            exp = ref.snap_row(x["cents"][0], x["f0"][0], [True], o, 0, 0xAB5)
            assert exp["v"][0] == half and int(info["notes"][0, 0]) == lower == int(exp["notes"][0]), (half, o)
            found += 1
            break
    assert found == 3
    # a frame exactly at the hysteresis limit stays; one unit less and it leaves
    a = np.float32((6000.0 + 4.0 - ref.K) / 7180.0)             # on C
    b = np.float32((6000.0 + 130.0 - ref.K) / 7180.0)           # nearer to D: 130 cents from C, 70 from D
    x = row_of([a, b])
    v = ref.position(b)
    h = abs(v - 60 * ref.S) - abs(v - 62 * ref.S)
    assert h > 0
    stats = TuningStatistics(offset=0, root=0, scale="major").to(device)
    for units, second in ((h, 60), (h - 1, 62), (h + 1, 60)):
        _, info = tune_pitch(z_of(x, device, keys=("cents", "f0")), stats, hysteresis=units / 65536.0, return_info=True)
        exp = ref.snap_row(x["cents"][0], x["f0"][0], [True, True], 0, 0, 0xAB5, h=units)
        assert info["notes"][0].tolist() == [60, second] == exp["notes"].tolist(), (units, info["notes"])
    # two offsets of equal cost go to the smaller |o|, then to the non-negative one
    cents_at = lambda c: np.float32((c - ref.K) / 7180.0)       # noqa: E731
    for deviations, offset in (([10, 20], 10), ([-20, -10], -10), ([-20] * 3 + [20] * 3 + [50], 20), ([-10, 10], 0)):
        x = row_of([cents_at(6000.0 + 100.0 * k + d) for k, d in enumerate(deviations)])
        stats = tuning_statistics(z_of(x, device, keys=("cents", "f0")), scale="chromatic")
        want = ref.statistics(x["cents"], [[True] * len(deviations)], mask=0xFFF)
        assert int(stats.offset[0]) == offset == int(want["offset"][0]) and int(stats.root[0]) == 0, (deviations, stats.offset)


def test_designed_ties():
    check_designed_ties("cpu")


def exact_cents(n):
    return 7180 * Fraction(float(n)) + Fraction(ref.K)


def check_hard_snap_and_second_pass(device, report=None):
    x = ref.make(41, 5, 172)
    stats, got = got_stats(x, device, {}, per_row=True)
    options = dict(vibrato=False, glide=0, amount=1.0)
    first = got_tune(x, device, stats, {}, **options)
    worst = (Fraction(0), Fraction(1))
    for b in range(5):
        o = int(got["offset"][b])
        on = first["notes"][b] != ref.OFF
        assert on.all()
        addend = (first["correction"][b].astype(np.float64) / (65536.0 * 7180.0)).astype(np.float32)
        ulp = lambda v: Fraction(float(np.spacing(np.abs(np.float32(v)))))    # noqa: E731
        for t in range(172):
            bound = 7180 * (ulp(first["cents"][b, t]) + ulp(addend[t])) / 2 + Fraction(1, 1 << 17)
            miss = abs(exact_cents(first["cents"][b, t]) - (100 * int(first["notes"][b, t]) + o))
            if first["correction"][b, t] == 0:
                bound = Fraction(1, 1 << 17)                    # (an untouched frame already lies on its note)
            assert miss <= bound, (b, t, float(miss), float(bound))
            if miss * worst[1] > worst[0] * bound:
                worst = (miss, bound)
    if report is not None:
        report.append((float(worst[0]), float(worst[1])))
    # the second pass changes no note and corrects by at most one rounding: the frame lies within the bound of its note, and
    # its position is rounded to a unit once more, so |d| <= 65536 bound + 1/2
    y = dict(x, cents=first["cents"], f0=first["f0"])
    second = got_tune(y, device, stats, {}, **options)
    assert same_bits(second["notes"], first["notes"])
    limit = 65536.0 * 7180.0 * 2.0 ** -24 + 1.0                 # ulp(n') <= 2^-23 below |n'| = 1, the addend's is smaller
    assert np.abs(y["cents"]).max() < 1.0 and np.abs(second["correction"]).max() <= limit, np.abs(second["correction"]).max()


def test_hard_snap_lands_within_the_bound_and_a_second_pass_is_idle():
    report = []
    check_hard_snap_and_second_pass("cpu", report)
    print("hard snap: worst miss %.3e cents at a bound of %.3e" % report[0])


def check_vibrato_kept(device):
    x = ref.make(42, 4, 172)
    stats, got = got_stats(x, device, {}, per_row=True)
    out = got_tune(x, device, stats, {}, vibrato=True, glide=0, amount=1.0)
    notes_seen = 0
    for b in range(4):
        o, t = int(got["offset"][b]), 0
        while t < 172:
            e = t
            while e + 1 < 172 and out["notes"][b, e + 1] == out["notes"][b, t]:
                e += 1
            c = out["correction"][b, t:e + 1]
            assert (c == c[0]).all()                            # vibrato kept: one correction for the whole note
            addend = np.float32(float(c[0]) / (65536.0 * 7180.0))
            ulp = lambda v: Fraction(float(np.spacing(np.abs(np.float32(v)))))            # noqa: E731
            bound = max(7180 * (ulp(n) + ulp(addend)) / 2 for n in out["cents"][b, t:e + 1]) + Fraction(1, 1 << 17)
            mean = sum(exact_cents(n) for n in out["cents"][b, t:e + 1]) / (e - t + 1)
            assert abs(mean - (100 * int(out["notes"][b, t]) + o)) <= bound, (b, t, e)
            # and the inflection: the frames' differences inside the note are the input's, up to the two roundings
            if e > t:
                din = np.diff(x["cents"][b, t:e + 1].astype(np.float64))
                dout = np.diff(out["cents"][b, t:e + 1].astype(np.float64))
                assert np.abs(din - dout).max() <= 2.0 ** -22
            notes_seen += 1
            t = e + 1
    assert notes_seen > 40


def test_vibrato_is_kept_and_note_means_land():
    check_vibrato_kept("cpu")


def check_identity_and_concert(device):
    x = ref.make(43, 3, 172, special=True)
    gate = GATES[1]
    stats, got = got_stats(x, device, gate, per_row=True)
    # amount = 0 returns n and f0 bit for bit, NaN payloads and signed zeros included
    x["cents"][0, 3], x["f0"][0, 4] = np.float32(-0.0), np.float32(-0.0)
    for amount in (0.0, np.zeros(3, dtype=np.float32)):
        out = got_tune(x, device, stats, gate, amount=amount, glide=2)
        assert same_bits(out["cents"], x["cents"]) and same_bits(out["f0"], x["f0"]) and not out["correction"].any()
    # concert=True differs from concert=False by exactly 65536 o on every frame of a corrected note
    for vibrato in (True, False):
        own = got_tune(x, device, stats, gate, min_note_frames=3, vibrato=vibrato)
        concert = got_tune(x, device, stats, gate, min_note_frames=3, vibrato=vibrato, concert=True)
        assert same_bits(own["notes"], concert["notes"])
        for b in range(3):
            notes, t, corrected = own["notes"][b], 0, np.zeros(172, dtype=bool)
            while t < 172:
                e = t
                while e + 1 < 172 and notes[e + 1] == notes[t]:
                    e += 1
                corrected[t:e + 1] = notes[t] != ref.OFF and e - t + 1 >= 3
                t = e + 1
            diff = own["correction"][b].astype(np.int64) - concert["correction"][b]
            assert np.array_equal(diff, np.where(corrected, 65536 * int(got["offset"][b]), 0)), (vibrato, b)
        assert not (own["notes"][1] != ref.OFF).any() and same_bits(own["cents"][1], x["cents"][1])      # a row with no on frame
    # off frames are never moved, whatever the options
    out = got_tune(x, device, stats, gate, glide=4, vibrato=False)
    off = out["notes"] == ref.OFF
    assert off.any() and same_bits(out["cents"][off], x["cents"][off]) and same_bits(out["f0"][off], x["f0"][off])
    assert not out["correction"][off].any()


def test_identity_concert_and_off_frames():
    check_identity_and_concert("cpu")


def check_melody(device):
    cents, played = ref.melody()
    x = dict(cents=cents, f0=ref.f0_of_cents(cents))
    z = z_of(x, device, keys=("cents", "f0"))
    stats = tuning_statistics(z)
    assert abs(int(stats.offset[0]) - 37) <= 1 and int(stats.root[0]) == 2 and int(stats.frames[0]) == 860
    assert int(tuning_statistics(z, scale="chromatic").root[0]) == 0          # every rotation of the chromatic mask ties
    new, info = tune_pitch(z, stats, hysteresis=20.0, return_info=True)
    assert np.array_equal(info["notes"][0].cpu().numpy(), played)
    # a second pass changes no note, and moves a note's frames by at most one rounding: each note's mean lies within the
    # hard-snap bound of its pitch, and the mean's quotient and the positions are rounded to a unit once more
    again, info2 = tune_pitch(new, stats, hysteresis=20.0, return_info=True)
    assert torch.equal(info2["notes"], info["notes"])
    assert int(info2["correction"].abs().max()) <= 65536.0 * 7180.0 * 2.0 ** -24 + 2.0
    # only f0: the wrapper derives normalized_cents first; tested for notes only
    _, info3 = tune_pitch({"f0": z["f0"]}, stats, return_info=True)
    assert np.array_equal(info3["notes"][0].cpu().numpy(), played)
    return int(stats.offset[0])


def test_melody_recovered():
    check_melody("cpu")


def test_statistics_object_and_errors():
    s = TuningStatistics(offset=0, root=2, scale="major")
    assert s.groups == 1 and s.mask == 0xAB5 and s.profile.shape == (1, 12) and s.frames.tolist() == [0]
    d = s.to_dict()
    t = TuningStatistics.from_dict(d).to("cpu")
    assert torch.equal(t.offset, s.offset) and torch.equal(t.root, s.root) and t.options() == s.options()
    assert TuningStatistics([3, -4], [0, 11], scale=0x091, silence=-2.0, confidence=0.5).options() == dict(scale=0x091, silence=-2.0, confidence=0.5)
    x = ref.make(44, 2, 9)
    z = z_of(x)
    for bad in (dict(scale="lydian"), dict(scale=0), dict(scale=0x1000), dict(root=12), dict(root=-1), dict(confidence=float("nan"))):
        with pytest.raises(ValueError):
            tuning_statistics(z, **bad)
    for bad in (dict(amount=1.5), dict(amount=-0.1), dict(amount=float("nan")), dict(hysteresis=-1.0), dict(hysteresis=1201.0),
                dict(min_note_frames=-1), dict(glide=-1), dict(glide=1.5), dict(scale=0), dict(root=12), dict(tuning=3),
                dict(tuning=TuningStatistics([0, 0, 0], [0, 0, 0])), dict(amount=torch.ones(3))):
        with pytest.raises(ValueError):
            tune_pitch(z, **bad)
    for bad in (dict(offset=51, root=0), dict(offset=0, root=12), dict(offset=[0, 0], root=[0])):
        with pytest.raises(ValueError):
            TuningStatistics(**bad)
    with pytest.raises(ValueError):
        tune_pitch({"harmonicity": z["harmonicity"]})
    with pytest.raises(ValueError):
        tune_pitch({"normalized_cents": z["normalized_cents"]})            # no f0 to move
    grad = dict(z, normalized_cents=z["normalized_cents"].clone().requires_grad_())
    with pytest.raises(Exception, match="grad"):
        tune_pitch(grad)
    with pytest.raises(Exception, match="grad"):
        tuning_statistics(grad)
    with pytest.raises(ValueError):
        ddsp.AutoEncoder.transfer(None, torch.zeros(1, 8), None, tune=3)


def test_symbols_constants_and_entry_point_validation():
    names = list(declared_prototypes())
    L = ctypes.CDLL(ddsp._lib.SO_PATH)
    for name in NEW_SYMBOLS:
        assert name in names and name in ddsp._lib.EXPORTS and name in ddsp._lib.SIGNATURES and hasattr(L, name), name
    at = names.index("ddsp_condition_apply")
    assert tuple(names[at + 1:at + 6]) == NEW_SYMBOLS and names[at + 6] == "ddsp_yin_salience"     # between section 10d and 10c
    assert list(ddsp._lib.SIGNATURES)[at + 1:at + 7] == list(NEW_SYMBOLS) + ["ddsp_yin_salience"]
    assert ddsp._lib.ABI_VERSION == 5 == ddsp._lib.lib().ddsp_hip_abi_version()
    assert ddsp.tune_pitch is tune_pitch and ddsp.tuning_statistics is tuning_statistics and ddsp.TuningStatistics is TuningStatistics
    assert {"tuning", "TuningStatistics", "tuning_statistics", "tune_pitch"} <= set(ddsp.__all__)
    # the literal against its formula, and the same literal everywhere
    assert abs(ref.K - (1997.3794084376191 - 1200.0 * math.log2(44.0) + 6900.0)) <= 2.0 ** -40
    assert ddsp.tuning.ORIGIN == ref.K and ddsp.tuning.SCALES == ref.SCALES and ddsp.tuning.OFF == ref.OFF
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ddsp_hip.h")).read()
    assert "K = 1997.3794084376191 - 1200 log2(44) + 6900 = 2346.0614660728625" in header
    L = ddsp._lib.lib()
    EINVAL, ERANGE = -1, -2
    word = (ctypes.c_uint64 * 8)()
    p = ctypes.addressof(word)
    assert L.ddsp_tuning_accum_bytes(1) == 4800 and L.ddsp_tuning_accum_bytes(7) == 7 * 4800 and L.ddsp_tuning_accum_bytes(0) == 0
    assert L.ddsp_tuning_workspace_bytes(3, ddsp.tuning.LDS_FRAMES) == 0
    assert L.ddsp_tuning_workspace_bytes(3, ddsp.tuning.LDS_FRAMES + 1) == 3 * (ddsp.tuning.LDS_FRAMES + 1) * 32
    stats = lambda rows, T, pooled=1, silence=0.0: L.ddsp_tuning_stats(p, None, None, None, p, rows, T, pooled, silence, 0.0, None)   # noqa: E731
    assert stats(0, 5) == 0 and stats(-1, 5) == EINVAL and stats(2, 0) == EINVAL and stats(2, 5, silence=float("nan")) == EINVAL
    assert L.ddsp_tuning_stats(None, None, None, None, p, 2, 5, 1, 0.0, 0.0, None) == EINVAL
    assert stats(1 << 16, 1 << 16) == ERANGE and stats(1, (1 << 24) + 1, 0) == ERANGE and stats(2, 1 << 24, 1) == ERANGE
    est = lambda groups, mask=0xAB5, root=-1: L.ddsp_tuning_estimate(p, p, p, p, p, groups, mask, root, None)       # noqa: E731
    assert est(0) == 0 and est(-1) == EINVAL and est(1, 0) == EINVAL and est(1, 0x1000) == EINVAL and est(1, 0xAB5, 12) == EINVAL
    assert L.ddsp_tuning_estimate(p, None, p, p, p, 1, 0xAB5, -1, None) == EINVAL

    def apply(B=1, T=5, groups=1, mask=0xAB5, root=-1, h=0, min_note=0, glide=0, flags=1, amount=1.0, silence=0.0, f0=p, work=None):
        return L.ddsp_tuning_apply(f0, p, None, None, None, p, p, None, p, p, None, None, work, B, T, groups, mask, root, h, min_note, glide,
                                   flags, amount, silence, 0.0, None)

    assert apply(B=0) == 0 and apply(B=-1) == EINVAL and apply(T=0) == EINVAL and apply(mask=0) == EINVAL and apply(root=12) == EINVAL
    assert apply(h=-1) == EINVAL and apply(h=1200 * 65536 + 1) == EINVAL and apply(min_note=-1) == EINVAL and apply(glide=-1) == EINVAL
    assert apply(flags=4) == EINVAL and apply(amount=1.5) == EINVAL and apply(amount=float("nan")) == EINVAL and apply(f0=None) == EINVAL
    assert apply(B=3, groups=2) == EINVAL and apply(silence=float("nan")) == EINVAL
    assert apply(T=1 << 24) == ERANGE and apply(B=1 << 12, T=1 << 19) == ERANGE
    assert apply(T=ddsp.tuning.LDS_FRAMES + 1) == EINVAL                          # a long row without its workspace
