"""CPU checks of `conditioning_statistics` and `fit_conditioning` (conditioning.py): the numpy path
against the plain-loop definitions of tests/conditioning_reference.py bit for bit, the consequences of the definitions, the C
entry points' declarations and their validation, and the containers."""
import ctypes
import functools
import inspect
import io

import numpy as np
import pytest
import torch

import ddsp_pytorch_amd as ddsp
import conditioning_reference as ref
from ddsp_pytorch_amd.conditioning import ConditioningStatistics, conditioning_statistics, fit_conditioning
from test_host_abi import declared_prototypes

NEW_SYMBOLS = ("ddsp_condition_accum_bytes", "ddsp_condition_launch_shape", "ddsp_condition_stats", "ddsp_condition_tables",
               "ddsp_condition_apply")
SHAPES = [(1, 1), (1, 2), (3, 5), (2, 63), (2, 64), (2, 65), (5, 172)]
QUANTILES, BINS = (1, 4, 64), (2, 64, 4096)
# (special values planted, a voiced mask, silence, confidence)
OPTIONS = [(False, False, None, 0.0), (True, True, -2.0, 0.3), (True, False, None, 0.5), (False, True, -1.0, 0.0)]
TARGET = (7, 4, 172)                                             # seed, rows, frames of the pooled target of the fit cases


def same_bits(a, b):
    """arrays of one dtype and shape equal bit for bit, NaNs compared as equal"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind != "f":
        return np.array_equal(a, b)
    word = np.uint32 if a.dtype == np.float32 else np.uint64
    nan_a, nan_b = np.isnan(a), np.isnan(b)
    return np.array_equal(nan_a, nan_b) and np.array_equal(a[~nan_a].view(word), b[~nan_b].view(word))


def z_of(x, device="cpu"):
    """the inputs of ref.make as the dict an Encoder returns"""
    names = dict(f0="f0", cents="normalized_cents", loud="loudness", harm="harmonicity", voiced="voiced")
    return {names[k]: torch.from_numpy(np.array(v))[..., None].to(device) for k, v in x.items()}


@functools.lru_cache(maxsize=None)
def inputs(seed, R, T, special=False, voiced=False):
    x = ref.make(seed, R, T, special=special, voiced=voiced)
    for v in x.values():
        v.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def want_stats(seed, R, T, special, voiced, per_row, Q, silence, confidence, bins):
    x = inputs(seed, R, T, special, voiced)
    return ref.statistics(x["loud"], x["cents"], x["harm"], x.get("voiced"), per_row=per_row, Q=Q, silence=silence,
                          confidence=confidence, bins=bins)


def got_stats(x, device="cpu", **kw):
    st, counts, sums = conditioning_statistics(z_of(x, device), return_histogram=True, **kw)
    return dict(counts=counts.cpu().numpy().astype(np.uint32), sums=sums.cpu().numpy(), tables=st.loudness_quantiles.cpu().numpy(),
                mean_pitch=st.mean_pitch.cpu().numpy(), mean_loudness=st.mean_loudness.cpu().numpy(), frames=st.frames.cpu().numpy())


def check_stats(got, exp, where):
    for k in ("counts", "sums", "tables", "mean_pitch", "mean_loudness", "frames"):
        assert same_bits(got[k], exp[k]), (where, k, got[k], exp[k])
    t = exp["tables"]
    finite = ~np.isnan(t).any(axis=1)
    assert (np.diff(t[finite], axis=1) >= 0).all(), (where, "a table that falls")
    assert np.isnan(t[~finite]).all() and (exp["frames"][~finite] == 0).all() and (exp["frames"][finite] > 0).all(), where


def stats_object(d, device="cpu", **options):
    """a reference dict as the package's container"""
    return ConditioningStatistics(torch.from_numpy(d["tables"]), torch.from_numpy(d["mean_pitch"]), torch.from_numpy(d["mean_loudness"]),
                                  torch.from_numpy(d["frames"]), **options).to(device)


def got_fit(x, target, device="cpu", **kw):
    new, info = fit_conditioning(z_of(x, device), target, return_info=True, **kw)
    return dict(f0=new["f0"][..., 0].cpu().numpy(), cents=new["normalized_cents"][..., 0].cpu().numpy(),
                loud=new["loudness"][..., 0].cpu().numpy(), octaves=info["octaves"].cpu().numpy(), frames=info["frames"].cpu().numpy())


def check_fit(got, exp, where):
    for k in ("f0", "cents", "loud", "octaves", "frames"):
        assert same_bits(got[k], exp[k]), (where, k, got[k], exp[k])


def case_seed(R, T, i):
    return 1000 * R + T + i


def run_cases(R, T, device):
    """every case of one shape: statistics pooled and per row, and the fit of the rows (each measured by itself, then through
    given statistics) to a pooled target, against the plain loops"""
    mapped = 0
    for Q in QUANTILES:
        for bins in BINS:
            for i, (special, voiced, silence, confidence) in enumerate(OPTIONS):
                seed = case_seed(R, T, i)
                x = inputs(seed, R, T, special, voiced)
                where = (R, T, Q, bins, i)
                for per_row in (False, True):
                    exp = want_stats(seed, R, T, special, voiced, per_row, Q, silence, confidence, bins)
                    check_stats(got_stats(x, device, per_row=per_row, quantiles=Q, silence=silence, confidence=confidence, bins=bins),
                                exp, where + (per_row,))
                source = want_stats(seed, R, T, special, voiced, True, Q, silence, confidence, bins)
                target = want_stats(*TARGET, False, False, False, Q, silence, confidence, bins)
                opts = dict(silence=silence, confidence=confidence, bins=bins)
                exp = ref.fit(x["f0"], x["cents"], x["loud"], source, target, min_frames=2, strength=0.75)
                tgt = stats_object(target, device, **opts)
                check_fit(got_fit(x, tgt, device, min_frames=2, strength=0.75), exp, where + ("measured",))
                check_fit(got_fit(x, tgt, device, source=stats_object(source, device, **opts), min_frames=2, strength=0.75), exp,
                          where + ("given",))
                mapped += int((exp["frames"] >= 2).sum())
    return mapped


def test_new_symbols_declared_exported_and_bound():
    names = list(declared_prototypes())
    L = ctypes.CDLL(ddsp._lib.SO_PATH)
    for name in NEW_SYMBOLS:
        assert name in names and name in ddsp._lib.EXPORTS and name in ddsp._lib.SIGNATURES and hasattr(L, name), name
    at = names.index("ddsp_pitch_voicing")
    assert tuple(names[at + 1:at + 6]) == NEW_SYMBOLS                              # section 10d follows 10b's voicing
    assert list(ddsp._lib.SIGNATURES)[at + 1:at + 6] == list(NEW_SYMBOLS)
    assert ddsp._lib.ABI_VERSION == 5 == ddsp._lib.lib().ddsp_hip_abi_version()      # adding symbols is compatible
    assert ddsp.conditioning_statistics is conditioning_statistics and ddsp.fit_conditioning is fit_conditioning
    assert ddsp.ConditioningStatistics is ConditioningStatistics
    assert {"conditioning", "ConditioningStatistics", "conditioning_statistics", "fit_conditioning"} <= set(ddsp.__all__)
    assert (ddsp.conditioning.MAX_BINS, ddsp.conditioning.MAX_QUANTILES) == (8192, 1024)
    assert float(ddsp.conditioning.VALUE_LIMIT) == float(ref.VALUE_LIMIT) and ddsp.conditioning.MAX_GROUP_FRAMES == ref.MAX_GROUP_FRAMES


def test_entry_points_validate_without_gpu():
    L = ddsp._lib.lib()
    word = ctypes.c_uint64(0)                      # (a valid address; nothing is read from it)
    p = ctypes.addressof(word)
    ninf = float("-inf")

    def stats(loud=p, cents=p, harm=p, accum=p, rows=1, T=8, pooled=0, bins=64, lo=-4.0, hi=2.0, silence=ninf, confidence=0.0):
        return L.ddsp_condition_stats(loud, cents, harm, None, accum, rows, T, pooled, bins, lo, hi, silence, confidence, None)

    for missing in ("loud", "cents", "harm", "accum"):
        assert stats(**{missing: None}) == -1, missing
    assert stats(rows=0) == 0 and stats(rows=0, loud=None, accum=None) == 0 and stats(rows=0, pooled=1) == 0    # an empty batch
    assert stats(rows=-1) == -1 and stats(T=0) == -1
    for bins in (0, -1, 8193):
        assert stats(bins=bins) == -1 and stats(bins=bins, rows=0) == -1
    assert stats(lo=2.0, hi=2.0) == -1 and stats(lo=2.0, hi=-4.0) == -1 and stats(hi=float("nan")) == -1
    assert stats(hi=float("inf")) == -1 and stats(lo=0.0, hi=1e-44, bins=8192) == -1          # a cell scale that is not finite
    assert stats(silence=float("nan")) == -1 and stats(confidence=float("nan")) == -1
    assert stats(rows=1 << 16, T=1 << 16) == -2 and stats(rows=1 << 16, T=1 << 16, pooled=1) == -2         # rows T >= 2^32
    assert stats(T=(1 << 24) + 1) == -2 and stats(rows=1 << 12, T=(1 << 12) + 1, pooled=1) == -2            # a group beyond 2^24

    def tables(accum=p, out=p, mp=p, ml=p, frames=p, groups=1, bins=64, Q=64, lo=-4.0, hi=2.0):
        return L.ddsp_condition_tables(accum, out, mp, ml, frames, groups, bins, Q, lo, hi, None)

    for missing in ("accum", "out", "mp", "ml", "frames"):
        assert tables(**{missing: None}) == -1, missing
    assert tables(groups=0) == 0 and tables(groups=0, accum=None) == 0 and tables(groups=-1) == -1
    for Q in (0, -1, 1025):
        assert tables(Q=Q) == -1 and tables(Q=Q, groups=0) == -1
    assert tables(bins=0) == -1 and tables(bins=8193) == -1 and tables(lo=1.0, hi=1.0) == -1

    names = ("f0", "cents", "loud", "S", "sm", "sf", "Tt", "tm", "f0_out", "cents_out", "loud_out")

    def apply(B=2, T=8, gs=1, gt=1, Q=64, mode=1, octaves=0, max_octaves=2, strength=1.0, min_frames=8, **ptr):
        a = {k: ptr.get(k, p) for k in names}
        return L.ddsp_condition_apply(a["f0"], a["cents"], a["loud"], a["S"], a["sm"], a["sf"], a["Tt"], a["tm"], None, a["f0_out"],
                                      a["cents_out"], a["loud_out"], None, None, B, T, gs, gt, Q, mode, octaves, max_octaves, strength,
                                      min_frames, None)

    for missing in names:
        assert apply(**{missing: None}) == -1, missing
    assert apply(B=0) == 0 and apply(B=0, f0=None) == 0 and apply(B=-1) == -1 and apply(T=0) == -1
    assert apply(gs=3) == -1 and apply(gt=0) == -1 and apply(Q=0) == -1 and apply(Q=1025) == -1
    assert apply(mode=3) == -1 and apply(mode=-1) == -1 and apply(max_octaves=-1) == -1 and apply(max_octaves=33) == -1
    assert apply(mode=2, octaves=33) == -1 and apply(strength=float("nan")) == -1
    assert apply(B=1 << 16, T=1 << 16) == -2 and apply(B=1 << 24, T=1) == -2

    blocks, unit = ctypes.c_int(0), ctypes.c_long(0)
    assert L.ddsp_condition_launch_shape(0, 3, 172, blocks, unit) == 0 and (blocks.value, unit.value) == (3, 172)
    assert L.ddsp_condition_launch_shape(0, 1 << 20, 5, blocks, unit) == 0
    cap = blocks.value
    assert 3 < cap < 1 << 20 and unit.value == 5                                   # more rows than workgroups: grid-strided
    assert L.ddsp_condition_launch_shape(1, 300, 7, blocks, unit) == 0 and blocks.value == -(-2100 // unit.value) >= 2
    assert L.ddsp_condition_launch_shape(0, 1, 1, None, unit) == -1 and L.ddsp_condition_launch_shape(0, 1 << 16, 1 << 16, blocks, unit) == -2
    assert L.ddsp_condition_accum_bytes(3, 7) == 88 + 48 and L.ddsp_condition_accum_bytes(1, 4096) == 4 * 4096 + 16
    assert L.ddsp_condition_accum_bytes(0, 64) == 0 and L.ddsp_condition_accum_bytes(1, 8193) == 0


def test_reference_pieces():
    assert ref.cell_of(np.float32(-4.0), -4.0, 2.0, 4096) == 0 and ref.cell_of(np.float32(-4.5), -4.0, 2.0, 4096) == 0
    assert ref.cell_of(np.float32(2.0), -4.0, 2.0, 4096) == 4095 and ref.cell_of(np.float32(7.25), -4.0, 2.0, 4096) == 4095
    assert ref.cell_of(np.float32(-1.0), -4.0, 2.0, 2) == 1 and ref.cell_of(np.float32(-1.5), -4.0, 2.0, 64) == 26
    f = np.float32
    assert not ref.is_on(f(np.nan), f(0), f(1), None, None, 0.0) and not ref.is_on(f(0), f(np.inf), f(1), None, None, 0.0)
    assert not ref.is_on(f(0), f(0), f(np.nan), None, None, 0.0) and ref.is_on(f(0), f(0), f(0), None, None, 0.0)
    assert not ref.is_on(f(-2), f(0), f(1), None, -2.0, 0.0) and ref.is_on(f(-1.99), f(0), f(1), None, -2.0, 0.0)     # strictly above
    assert not ref.is_on(f(0), f(0), f(1), False, None, 0.0) and not ref.is_on(f(1e30), f(0), f(1), None, None, 0.0)
    # four frames in cells 0, 0, 1, 3 of four: quantiles at a quarter of the way each
    S = ref.quantile_table([2, 1, 0, 1], 4, 0.0, 4.0)
    assert S.tolist() == [0.0, 0.5, 1.0, 2.0, 4.0]
    assert np.isnan(ref.quantile_table([0, 0], 3, 0.0, 1.0)).all()
    assert ref.octave_shift(0.6, 0.6 - 1230 / 7180) == 1 and ref.octave_shift(0.5, float("nan")) == 0
    assert ref.octave_shift(0.5, 0.5 - 2.5 * 1200 / 7180, max_octaves=5) in (2, 3) and ref.octave_shift(0.0, 1.0, octaves=-4) == -4


@pytest.mark.parametrize("R,T", SHAPES)
def test_cpu_equals_reference_bit_for_bit(R, T):
    mapped = run_cases(R, T, "cpu")
    assert mapped > 0 or T < 2


def test_inputs_reach_every_mechanism():
    """the seeded maker gives rows without an on frame, fewer on frames than quantiles, values below lo, at hi and above it,
    NaN and both infinities in each input, and frames that each gate alone switches off"""
    x = inputs(case_seed(5, 172, 1), 5, 172, True, True)
    assert (x["loud"] < -4).any() and (x["loud"] == 2.0).any() and (x["loud"] > 2.0).any()
    for k in ("loud", "cents", "harm", "f0"):
        assert np.isnan(x[k]).any() and np.isinf(x[k]).any(), k
    assert np.isneginf(x["loud"]).any() and np.isneginf(x["cents"]).any() and np.isneginf(x["harm"]).any()
    st = want_stats(case_seed(5, 172, 1), 5, 172, True, True, True, 64, -2.0, 0.3, 4096)
    assert st["frames"][0] == 0 and (st["frames"][1:] > 0).all() and st["counts"][:, 0].sum() == 0
    everything = want_stats(case_seed(5, 172, 2), 5, 172, True, False, True, 64, None, 0.0, 4096)
    assert everything["counts"][1:, 0].all() and everything["counts"][1:, -1].min() >= 2          # below lo; hi and above it
    few = want_stats(case_seed(3, 5, 0), 3, 5, False, False, True, 64, None, 0.0, 4096)
    assert (few["frames"] < 64).all() and (few["frames"] > 0).all()                               # N < Q
    gates = [want_stats(case_seed(5, 172, 3), 5, 172, False, True, False, 4, s, c, 64)["frames"][0]
             for s, c in ((None, 0.0), (-1.0, 0.0), (None, 0.4))]
    plain = ref.statistics(*(inputs(case_seed(5, 172, 3), 5, 172, False, True)[k] for k in ("loud", "cents", "harm")), Q=4, bins=64)
    assert gates[1] < gates[0] < plain["frames"][0] and gates[2] < gates[0]


def inside(l, S):
    return np.isfinite(l) & (l >= S[0]) & (l < S[-1])


def identity_bound(l, S):
    """4 * 2^-24 * max(|S_k|, |S_k+1|) of the finite frames inside the table, their mask"""
    m = inside(l, S)
    k = np.minimum(np.searchsorted(S, l[m], side="right") - 1, len(S) - 2)
    return m, 4.0 * 2.0 ** -24 * np.maximum(np.abs(S[k].astype(np.float64)), np.abs(S[k + 1].astype(np.float64)))


IDENTITY = [(31, 3, 172, True), (32, 1, 700, False), (33, 2, 65, True), (34, 2, 700, True)]


@functools.lru_cache(maxsize=None)
def identity_inputs(seed, R, T, special):
    """`inputs` with the loudness moved off its grid of 1/64, so that the map's roundings show; and its per-row statistics"""
    x = dict(inputs(seed, R, T, special))
    x["loud"] = (x["loud"].astype(np.float64) * 0.98765 + 0.00377).astype(np.float32)
    return x, {Q: ref.statistics(x["loud"], x["cents"], x["harm"], per_row=True, Q=Q) for Q in (1, 4, 64)}


def check_identity(got, x, tables, where):
    """a performance fitted to its own statistics: no octave, the loudness within the bound inside the table and untouched
    outside it"""
    assert not got["octaves"].any(), where
    worst, outside = 0.0, 0
    for r in range(len(tables)):
        l, S = x["loud"][r], tables[r]
        m, bound = identity_bound(l, S)
        err = np.abs(got["loud"][r][m].astype(np.float64) - l[m].astype(np.float64))
        assert (err <= bound).all(), (where, r, float((err / bound).max()))
        worst = max(worst, float((err * 2.0 ** 24).max(initial=0.0)))
        assert same_bits(got["loud"][r][~m], l[~m]), (where, r, "outside the table")
        assert m.any() or np.isnan(S).all(), where
        outside += int((np.isfinite(l) & ~m).sum())
    assert outside or where[1] == 32, where                       # (the planted values lie outside; seed 32 has none)
    return worst


@pytest.mark.parametrize("Q", [1, 4, 64])
def test_fit_to_its_own_statistics_is_the_identity(Q):
    for seed, R, T, special in IDENTITY:
        x, own = identity_inputs(seed, R, T, special)
        own = own[Q]
        # the definition by itself first: the bound is a statement about the arithmetic, not about the package
        exp = ref.fit(x["f0"], x["cents"], x["loud"], own, own)
        worst = check_identity(exp, x, own["tables"], ("reference", seed, Q))
        print(f"identity, Q = {Q}, {R} x {T}: the reference is at most {worst:.2f} * 2^-24 off")
        target = conditioning_statistics(z_of(x), per_row=True, quantiles=Q)
        got = got_fit(x, target, octaves=True)
        check_identity(got, x, own["tables"], ("cpu", seed, Q))
        check_fit(got, exp, ("cpu", seed, Q))
        assert same_bits(got["f0"], x["f0"]) and same_bits(got["cents"], x["cents"])


def hand_made(S, Tt, mean_source=0.5, mean_target=0.5):
    return (ConditioningStatistics(torch.tensor([S]), torch.tensor([mean_source])),
            ConditioningStatistics(torch.tensor([Tt]), torch.tensor([mean_target])))


def test_hand_made_tables_with_flat_segments():
    """Flat segments in either table: the map follows the definition bit for bit and never falls.  With a non-decreasing
    source table the frame's segment ends above the frame (S[k] <= l < S[k + 1]), so its width is positive: the definition's
    0.5 weight is reached only through a table that falls, and is checked there too."""
    S = [-3.0, -2.0, -2.0, -2.0, -1.0, -1.0, 0.5, 0.5]
    Tt = [-2.5, -2.5, -2.0, -1.0, -1.0, 0.0, 0.0, 1.0]
    source, target = hand_made(S, Tt)
    edges = np.array(S + Tt, dtype=np.float32)
    l = np.sort(np.concatenate([np.linspace(-4, 1.5, 397).astype(np.float32), edges, np.nextafter(edges, np.float32(-9)),
                                np.nextafter(edges, np.float32(9))]))[None]
    x = dict(f0=np.full_like(l, 220.0), cents=np.full_like(l, 0.5), loud=l, harm=np.ones_like(l))
    got = got_fit(x, target, source=source)
    exp = ref.fit(x["f0"], x["cents"], x["loud"], dict(tables=np.array([S], np.float32), mean_pitch=[0.5], frames=[99]),
                  dict(tables=np.array([Tt], np.float32), mean_pitch=[0.5], frames=[99]))
    assert same_bits(got["loud"], exp["loud"]) and not got["octaves"].any()
    assert (np.diff(got["loud"][0]) >= 0).all()                                     # monotone across the flat segments
    at = lambda v: got["loud"][0][l[0] == np.float32(v)][0]                         # noqa: E731
    assert at(-2.0) == np.float32(-1.0) and at(-1.0) == np.float32(0.0)             # the last entry of a flat run decides
    assert at(-3.0) == np.float32(-2.5) and at(0.5) == np.float32(1.0) and at(1.5) == np.float32(2.0) and at(-4.0) == np.float32(-3.5)
    below = got["loud"][0][l[0] == np.nextafter(np.float32(-2.0), np.float32(-9))][0]
    assert below <= np.float32(-2.5) + np.float32(1e-6)                             # ... and the first one the frames below it
    # the 0.5 weight of a segment without width, straight from the definition
    assert ref.map_loudness(np.float32(-2.0), np.array([-3, -2, -2, -1], np.float32), np.array([0, 1, 2, 3], np.float32)) == 2.0
    flat = np.array([1.0, 1.0], np.float32)
    assert ref.map_loudness(np.float32(1.0), flat, np.array([5.0, 7.0], np.float32)) == 7.0   # at S[Q]: the shift of the end


def pitch_case(cents_below, T=16):
    """one row whose frames all sit `cents_below` under a target mean of 0.6"""
    n = np.full((1, T), np.float32(0.6 - cents_below / 7180.0))
    rng = np.random.default_rng(abs(int(cents_below)))
    return dict(f0=(110.0 + rng.random((1, T))).astype(np.float32), cents=n, loud=(-2.0 + rng.random((1, T))).astype(np.float32),
                harm=np.ones((1, T), np.float32))


def check_pitch(device="cpu"):
    target = ConditioningStatistics(torch.linspace(-3, 0, 65)[None], torch.tensor([0.6])).to(device)
    for cents_below, kw, k in ((1230, {}, 1), (1810, dict(max_octaves=3), 2), (1810, {}, 2), (3000, {}, 2), (-1230, {}, -1),
                               (3000, dict(max_octaves=1), 1), (3100, dict(max_octaves=4), 3), (1230, dict(octaves=False), 0),
                               (1230, dict(octaves=-3), -3), (100, {}, 0)):
        x = pitch_case(cents_below)
        got = got_fit(x, target, device, **kw)
        assert got["octaves"].tolist() == [k], (cents_below, kw, got["octaves"])
        assert same_bits(got["f0"], x["f0"] * np.float32(2.0 ** k))                 # exactly f0 2^k
        assert same_bits(got["cents"], x["cents"] + np.float32(k * 1200.0 / 7180.0))
        src = ref.statistics(x["loud"], x["cents"], x["harm"], per_row=True)
        exp = ref.fit(x["f0"], x["cents"], x["loud"], src, dict(tables=target.loudness_quantiles.cpu().numpy(), mean_pitch=[0.6], frames=[99]),
                      **kw)
        check_fit(got, exp, (cents_below, kw))


def test_octave_shift_rounds_then_clamps():
    check_pitch()


def check_strength(device="cpu"):
    x = inputs(41, 3, 172)
    target = stats_object(want_stats(*TARGET, False, False, False, 64, None, 0.0, 4096), device)
    full = got_fit(x, target, device, octaves=False)
    assert not same_bits(full["loud"], x["loud"])
    none = got_fit(x, target, device, octaves=False, strength=0.0)
    assert same_bits(none["loud"], x["loud"]) and same_bits(none["f0"], x["f0"]) and same_bits(none["cents"], x["cents"])
    rows = torch.tensor([0.0, 1.0, 0.25], device=device)
    mixed = got_fit(x, target, device, octaves=False, strength=rows)
    quarter = got_fit(x, target, device, octaves=False, strength=0.25)
    assert same_bits(mixed["loud"][0], x["loud"][0]) and same_bits(mixed["loud"][1], full["loud"][1])
    assert same_bits(mixed["loud"][2], quarter["loud"][2]) and not same_bits(quarter["loud"][2], full["loud"][2])
    src = want_stats(41, 3, 172, False, False, True, 64, None, 0.0, 4096)
    exp = ref.fit(x["f0"], x["cents"], x["loud"], src, want_stats(*TARGET, False, False, False, 64, None, 0.0, 4096), octaves=False,
                  strength=[0.0, 1.0, 0.25])
    check_fit(mixed, exp, "per-row strength")


def test_strength_mixes_rows_independently():
    check_strength()


def min_frames_case():
    x = {k: v.copy() for k, v in inputs(43, 2, 40).items()}
    x["cents"][0, 7:] = np.nan                                    # 7 on frames
    x["cents"][1, 8:] = np.nan                                    # 8
    return x


def check_min_frames(device="cpu"):
    x = min_frames_case()
    target = stats_object(want_stats(*TARGET, False, False, False, 64, None, 0.0, 4096), device)
    got = got_fit(x, target, device, octaves=1)
    assert got["frames"].tolist() == [7, 8] and got["octaves"].tolist() == [0, 1]
    for k in ("f0", "cents", "loud"):
        assert same_bits(got[k][0], x[k][0]), k                   # the row as it came
    assert same_bits(got["f0"][1], x["f0"][1] * np.float32(2)) and not same_bits(got["loud"][1], x["loud"][1])
    assert got_fit(x, target, device, octaves=1, min_frames=7)["octaves"].tolist() == [1, 1]
    # a table with a NaN in it is too little to go on as well
    broken = target.loudness_quantiles.clone()
    broken[0, 5] = float("nan")
    got = got_fit(x, ConditioningStatistics(broken, target.mean_pitch), device, octaves=1)
    assert got["octaves"].tolist() == [0, 0] and all(same_bits(got[k], x[k]) for k in ("f0", "cents", "loud"))


def test_min_frames_leaves_a_row_unchanged():
    check_min_frames()


def test_pooled_statistics_do_not_depend_on_the_order_of_the_rows():
    x = inputs(case_seed(5, 172, 1), 5, 172, True, True)
    perm = np.random.default_rng(3).permutation(5)
    a = got_stats(x, quantiles=64, silence=-2.0, confidence=0.3)
    b = got_stats({k: v[perm] for k, v in x.items()}, quantiles=64, silence=-2.0, confidence=0.3)
    for k in a:
        assert torch.equal(torch.from_numpy(a[k].astype(np.int64) if a[k].dtype == np.uint32 else a[k]).nan_to_num(nan=-77.0),
                           torch.from_numpy(b[k].astype(np.int64) if b[k].dtype == np.uint32 else b[k]).nan_to_num(nan=-77.0)), k
    assert a["frames"][0] > 100


def test_to_dict_round_trip_and_container():
    x = inputs(41, 3, 172)
    st = conditioning_statistics(z_of(x), per_row=True, quantiles=4, silence=-3.0, confidence=0.25, lo=-5.0, hi=3.0, bins=64)
    d = st.to_dict()
    assert set(d) == {"loudness_quantiles", "mean_pitch", "mean_loudness", "frames", "lo", "hi", "bins", "silence", "confidence"}
    assert all(isinstance(d[k], torch.Tensor) for k in ("loudness_quantiles", "mean_pitch", "mean_loudness", "frames"))
    assert (d["lo"], d["hi"], d["bins"], d["silence"], d["confidence"]) == (-5.0, 3.0, 64, -3.0, 0.25)
    buf = io.BytesIO()
    torch.save(d, buf)
    buf.seek(0)
    back = ConditioningStatistics.from_dict(torch.load(buf, weights_only=True))
    for k in ("loudness_quantiles", "mean_pitch", "mean_loudness", "frames"):
        assert torch.equal(getattr(back, k), getattr(st, k)) and getattr(back, k).dtype == getattr(st, k).dtype, k
    assert back.options() == st.options() and (back.groups, back.quantiles) == (3, 4)
    assert st.mean_pitch.dtype == st.mean_loudness.dtype == torch.float64 and st.frames.dtype == torch.int64
    assert st.loudness_quantiles.dtype == torch.float32 and st.to("cpu").options() == st.options()
    assert conditioning_statistics(z_of(x)).to_dict()["silence"] is None
    # by hand: a single table is one group, counted as well measured
    hand = ConditioningStatistics([-3.0, -1.0, 0.0], 0.5)
    assert (hand.groups, hand.quantiles) == (1, 2) and int(hand.frames[0]) >= 8 and torch.isnan(hand.mean_loudness).all()
    with pytest.raises(ValueError):
        ConditioningStatistics([[1.0]], [0.5])
    with pytest.raises(ValueError):
        ConditioningStatistics([[1.0, 2.0], [1.0, 2.0]], [0.5])


def test_argument_validation():
    x = inputs(41, 3, 172)
    z = z_of(x)
    target = conditioning_statistics(z)
    for bad in (dict(quantiles=0), dict(quantiles=1025), dict(bins=0), dict(bins=8193), dict(lo=1.0, hi=1.0), dict(lo=2.0, hi=-4.0),
                dict(silence=float("nan")), dict(confidence=float("nan")), dict(voiced=torch.ones(3, 172, 1)),
                dict(voiced=torch.ones(3, 171, 1, dtype=torch.bool))):
        with pytest.raises(ValueError):
            conditioning_statistics(z, **bad)
    with pytest.raises(ValueError):
        conditioning_statistics({k: v for k, v in z.items() if k != "harmonicity"})
    with pytest.raises(ValueError):
        conditioning_statistics(dict(z, loudness=z["loudness"][..., 0]))
    with pytest.raises(ValueError):
        conditioning_statistics(dict(z, loudness=z["loudness"][:, :100]))
    with pytest.raises(RuntimeError, match="no backward"):
        conditioning_statistics(dict(z, loudness=z["loudness"].clone().requires_grad_()))
    big = torch.zeros(1, (1 << 24) + 1, 1)
    with pytest.raises(ValueError, match="2\\^24"):                                 # the int64 sums: refused, not wrapped
        conditioning_statistics(dict(loudness=big, normalized_cents=big, harmonicity=big))
    for bad in (dict(octaves=2.5), dict(octaves=33), dict(max_octaves=-1), dict(max_octaves=40), dict(min_frames=-1),
                dict(strength=float("nan")), dict(strength=torch.ones(2)), dict(source=conditioning_statistics(z, quantiles=4)),
                dict(source=conditioning_statistics(z_of(inputs(43, 2, 40)), per_row=True)), dict(source="own")):
        with pytest.raises(ValueError):
            fit_conditioning(z, target, **bad)
    with pytest.raises(ValueError):
        fit_conditioning(z, "violin")
    with pytest.raises(ValueError):
        fit_conditioning({k: v for k, v in z.items() if k != "f0"}, target)
    new = fit_conditioning(dict(z, extra=z["harmonicity"]), target)
    assert list(new) == list(z) + ["extra"] and new["extra"] is z["harmonicity"] and new["harmonicity"] is z["harmonicity"]
    assert all(new[k] is not z[k] and new[k].shape == z[k].shape and new[k].dtype == torch.float32
               for k in ("f0", "normalized_cents", "loudness"))
    _, info = fit_conditioning(z, target, return_info=True)
    assert info["octaves"].dtype == torch.int32 and info["frames"].dtype == torch.int64 and info["octaves"].shape == (3,)
    # z's own mask is used when none is passed
    masked = dict(z, voiced=torch.from_numpy(np.ascontiguousarray(x["loud"] > -1.5))[..., None])
    assert torch.equal(conditioning_statistics(masked).frames, conditioning_statistics(z, voiced=masked["voiced"]).frames)
    assert int(conditioning_statistics(masked).frames) < int(target.frames)
    assert "not tuned" in conditioning_statistics.__doc__ and "2^63" in conditioning_statistics.__doc__


def test_autoencoder_hooks_are_additive():
    sig = inspect.signature(ddsp.AutoEncoder.forward_live)
    assert list(sig.parameters) == ["self", "x", "hidden", "delayed", "conditioning"]
    assert sig.parameters["conditioning"].default is None and sig.parameters["delayed"].default is False
    assert list(inspect.signature(ddsp.AutoEncoder.transfer).parameters) == ["self", "x", "target", "fit_options"]
