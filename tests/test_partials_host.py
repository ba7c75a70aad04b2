"""The inharmonic analysis without a device: the torch-op path of partials.py against the fp64 definition of
tests/partials_reference.py, the properties of the method on stiff strings built with the bank's own forward, the closed-form fit,
the cross-check with the harmonic analysis of section 14, masks, the wiring, and the usability of the device bounds.  The library
is used for the entry checks that need no device only.  Every figure is printed before it is asserted."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ddsp_pytorch_amd as ddsp
import harmonic_analysis_reference as ref
import partials_reference as pr
from sinusoids_reference import EPS64

SR, HOP, W = 16000, 128, 1024
T_STRING = 40
# Twice what the fp64 reference itself leaves on the K = 12 string (f0 110 Hz, B 3e-4, weights 1 / k) analysed along its true
# tracks: 1.473e-3 of the weakest partials' amplitude and 2.733e-4 of the rms -- Hann side-lobe leakage between the partials, not
# rounding (recorded in DESIGN.md section 14e).
CAP_AMPLITUDE = 2 * 1.473e-3
CAP_RESIDUAL = 2 * 2.733e-4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def t64(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))


# ---- 1. the torch path is the definition -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 12, 16, 64, 5, 16000), (2, 12, 7, 64, 5, 16000)])
def test_torch_path_against_the_definition_in_fp64(shape):
    """Tolerance, counted: the phase is a fp64 prefix here and a longdouble one in the reference, E_P = (T + 8) 2^-53 (|P| + 1) turns
    for each; cos / sin of the fp64 angle and the product 2 pi turns a few 2^-53; the W terms of an element summed in fp64 in some
    order, W 2^-53 sum |w x|.  So an element of the unscaled sums is within sqrt(2) sum_j |x_j| (4 pi E_P + (W + 16) 2^-53), and
    f_re within the first-order propagation of that through num / den plus 8 ulps of f for the window mean."""
    B, T, hop, Wn, K, sr = shape
    audio, f, voiced = pr.string_rows(*shape)
    a64, f64 = audio.astype(np.float64), f.astype(np.float64)
    got = ddsp.partial_analysis(t64(a64), t64(f64), hop, sr, Wn, voiced=torch.from_numpy(voiced)[..., None], return_complex=True,
                                reassign=True)
    harm, resid, again = ddsp.partial_residual(t64(a64), t64(f64), hop, sr, Wn, voiced=torch.from_numpy(voiced)[..., None],
                                               return_complex=True)
    assert sorted(got) == ["C", "a", "c", "f", "f_re"] and got["C"].dtype == torch.complex128 and sorted(again) == ["C", "a", "c", "f"]
    assert torch.equal(got["C"], again["C"]) and torch.equal(resid, t64(a64) - harm)
    w, wd = pr.windows(Wn)
    worst = np.zeros(5)
    for b in range(B):
        want = pr.analyse(a64[b], f64[b], hop, sr, Wn, voiced[b], cast=False)
        e_p = (T + 8) * EPS64 * (np.abs(pr.phases(f64[b], hop, sr, cast=False)).max() + 1.0)
        per_term = 4 * np.pi * e_p + (Wn + 16) * EPS64
        tol_C = np.zeros(T)
        tol_f = np.full((T, K), np.inf)
        for t in range(T):
            n = ref.frame_start(t, hop, Wn) + np.arange(Wn)
            inside = (n >= 0) & (n < T * hop)
            x = a64[b][n[inside]]
            sx, sd = np.abs(w[inside] * x).sum(), np.abs(wd[inside] * x).sum()
            tol_C[t] = np.sqrt(2.0) * per_term * sx * 2.0 / w[inside].sum()
            bC, bD = np.sqrt(2.0) * per_term * sx, np.sqrt(2.0) * per_term * sd
            aC, aD = np.abs(want["Cu"][t]), np.abs(want["Du"][t])
            with np.errstate(invalid="ignore", divide="ignore"):
                q = np.abs((want["Du"][t] * np.conj(want["Cu"][t])).imag) / aC ** 2
                tol_f[t] = sr / (2 * np.pi) * 2 * (aD * bC + aC * bD + q * 2 * aC * bC) / aC ** 2 + 8 * EPS64 * np.abs(f64[b][t])
        C = got["C"][b].numpy()
        m = want["measured"]
        assert np.array_equal(got["f_re"][b].numpy()[~m], f64[b][~m], equal_nan=True)          # not defined: the entry itself
        assert not C[~want["keep"]].any()
        assert np.array_equal(got["f"][b].numpy(), np.where(pr.usable(f64[b]), f64[b], 0.0))
        strong = m & (np.abs(want["C"]) >= 1e-3 * np.abs(want["C"]).max())
        h, _ = pr.resynth(C, f64[b], hop, sr, cast=False)
        worst = np.maximum(worst, [(np.abs(C - want["C"]).max(axis=-1) / tol_C).max(),
                                   (np.abs(got["a"][b, :, 0].numpy() - want["a"]) / (K * tol_C)).max(),
                                   np.abs(got["c"][b].numpy() - want["c"]).max() / 1e-12,
                                   (np.abs(got["f_re"][b].numpy() - want["f_re"])[strong] / tol_f[strong]).max(),
                                   np.abs(harm[b].numpy() - h).max() / (K * per_term * np.abs(C).max() + 1e-300)])
    print(f"{shape}: error / counted fp64 tolerance: C {worst[0]:.3f}, a {worst[1]:.3f}, c / 1e-12 {worst[2]:.3f}, f_re {worst[3]:.3f}, "
          f"harm {worst[4]:.3f}")
    assert worst.max() <= 1.0


# ---- 2. the method ------------------------------------------------------------------------------------------------------------------
def test_a_string_analysed_along_its_true_tracks_returns_its_controls():
    y, f, amps = pr.string_tone(110.0, 3e-4, 12, T_STRING, HOP, SR)
    inter = pr.interior_frames(T_STRING, HOP, W)
    want = pr.analyse(y, f, HOP, SR, W, cast=False)
    h, _ = pr.resynth(want["C"], f, HOP, SR, cast=False)
    ref_amp = (np.abs(np.abs(want["C"][inter]) - amps) / amps).max()
    ref_res = pr.residual_share(y, y - h, T_STRING, HOP, W)
    harm, resid, got = ddsp.partial_residual(t64(y)[None], t64(f)[None], HOP, SR, W, return_complex=True)
    amp = (np.abs(got["C"][0].abs().numpy()[inter] - amps) / amps).max()
    ac = (np.abs((got["a"] * got["c"])[0].numpy()[inter] - amps) / amps).max()
    res = pr.residual_share(y, resid[0].numpy(), T_STRING, HOP, W)
    print(f"K 12 string along its true tracks: |C| off a c by {amp:.3e} (reference {ref_amp:.3e}, cap {CAP_AMPLITUDE:.3e}); "
          f"residual {res:.3e} of the rms (reference {ref_res:.3e}, cap {CAP_RESIDUAL:.3e})")
    assert 2 * ref_amp <= CAP_AMPLITUDE * 1.001 and 2 * ref_res <= CAP_RESIDUAL * 1.001          # the caps are what they say they are
    assert amp <= CAP_AMPLITUDE and ac <= CAP_AMPLITUDE and res <= CAP_RESIDUAL


def _fit_string(f0, B_coef, K, iterations=4):
    y, f, _ = pr.string_tone(f0, B_coef, K, T_STRING, HOP, SR)
    start = torch.full((1, T_STRING, 1), f0 * 1.004, dtype=torch.float64)
    d = ddsp.inharmonic_analysis(t64(y)[None], start, HOP, SR, K, W, inharmonicity=0.0, iterations=iterations)
    assert sorted(d) == ["a", "c", "f0", "inharmonicity", "ratios"] and d["ratios"].shape == (1, T_STRING, K)
    assert d["inharmonicity"].shape == (1,) and d["f0"].shape == (1, T_STRING, 1)
    model = (d["f0"] * d["ratios"])[0].numpy()
    off = np.abs(pr.cents(model, f)).max()
    return y, f, model, off, abs(float(d["inharmonicity"][0]) / B_coef - 1.0)


def test_the_loop_finds_a_stiff_string_from_a_harmonic_start():
    """f0 110 Hz, B 3e-4, K 24, started at B = 0 and 0.4 % sharp (the top partial 140 cents off): after four steps the model track is
    within 1 cent of the truth on every partial and B within 2 % (measured: 0.026 cents, 0.001 %).  And the reason the feature
    exists: the harmonic analysis of the same string leaves at least 10 times the residual rms (measured: 0.176 against 3.0e-4,
    591 times; the fp64 references alone: 597 times)."""
    y, f, model, off, rel = _fit_string(110.0, 3e-4, 24)
    print(f"110 Hz, B 3e-4, K 24 after 4 steps: {off:.4f} cents off at most, B off by {100 * rel:.4f} %")
    assert off <= 1.0 and rel <= 0.02
    _, resid, _ = ddsp.partial_residual(t64(y)[None], t64(model)[None], HOP, SR, W)
    _, resid_h, _ = ddsp.harmonic_residual(t64(y)[None], torch.full((1, T_STRING, 1), 110.0, dtype=torch.float64), HOP, SR, 24, W)
    inharmonic, harmonic = (pr.residual_share(y, r[0].numpy(), T_STRING, HOP, W) for r in (resid, resid_h))
    want = pr.analyse(y, f, HOP, SR, W, cast=False)
    Ch, _, _ = ref.analyse(y, np.full(T_STRING, 110.0), HOP, SR, 24, W)
    ref_in = pr.residual_share(y, y - pr.resynth(want["C"], f, HOP, SR, cast=False)[0], T_STRING, HOP, W)
    ref_h = pr.residual_share(y, y - ref.resynth(Ch, np.full(T_STRING, 110.0), HOP, SR), T_STRING, HOP, W)
    print(f"residual rms / signal rms: inharmonic {inharmonic:.3e}, harmonic {harmonic:.3e}, ratio {harmonic / inharmonic:.1f}; "
          f"the references alone: {ref_in:.3e}, {ref_h:.3e}, ratio {ref_h / ref_in:.1f}")
    assert ref_h >= 10 * ref_in and harmonic >= 10 * inharmonic


def test_the_loop_finds_a_stiffer_string():
    """f0 220 Hz, B 1e-3, K 16 under the same conditions: within 1 cent and 2 % after four steps (measured: 0.54 cents, 0.30 %).
    This is the harder start: with f0 0.4 % sharp and B = 0 the model's partial 14 (3092.3 Hz) lies on the string's partial 13
    (3092.2 Hz) and is measured with that partial's full amplitude, which holds the |C|^2-weighted fit back for three steps; the
    fourth is the first with every partial on its own line (after three steps: 115 cents; after six: 0.02 cents)."""
    _, _, _, off, rel = _fit_string(220.0, 1e-3, 16)
    print(f"220 Hz, B 1e-3, K 16 after 4 steps: {off:.4f} cents off at most, B off by {100 * rel:.4f} %")
    assert off <= 1.0 and rel <= 0.02


def test_the_free_model_keeps_every_partial_on_its_own_track():
    """A bell: ratios that no stiff string has.  model='free' returns the measured tracks, model='stiff' cannot."""
    K, ratios = 4, np.array([1.0, 2.76, 5.4, 8.93])
    f = np.tile(200.0 * ratios, (T_STRING, 1))
    import sinusoids_reference as sref
    y = sref.forward(f[None], np.ones((1, T_STRING, K)), np.full((1, T_STRING, 1), 0.5), HOP, SR, cast=False)["y"][0]
    start = np.tile(200.0 * ratios * 2.0 ** (np.array([3.0, -6.0, 8.0, -4.0]) / 1200.0), (T_STRING, 1))
    refined = ddsp.refine_partials(t64(y)[None], t64(start)[None], HOP, SR, W, iterations=2)
    off = np.abs(pr.cents(refined[0].numpy(), f)).max()
    d = ddsp.inharmonic_analysis(t64(y)[None], torch.full((1, T_STRING, 1), 200.6, dtype=torch.float64), HOP, SR, K, W,
                                 base_ratios=ratios * np.array([1.0, 1.002, 0.997, 1.003]), iterations=3, model='free')
    free = np.abs(pr.cents((d["f0"] * d["ratios"])[0].numpy(), f)).max()
    print(f"bell: refine_partials from up to 8 cents off: {off:.4f} cents; inharmonic_analysis(model='free'): {free:.4f} cents")
    # the property: the measured tracks are an order of magnitude closer than the 8 cents (and 5 cents) they started from; what is
    # left (0.16 cents here) is the leakage of the other partials into a 64 ms window, as in the K = 12 string above
    assert off <= 0.8 and free <= 0.5
    held = ddsp.refine_partials(t64(y)[None], t64(start)[None], HOP, SR, W, iterations=2, max_cents=2.0)
    moved = np.abs(pr.cents(held[0].numpy(), start))
    assert moved.max() <= 2.0 + 1e-9 and moved.max() >= 2.0 - 1e-9                              # the clamp is reached and held


# ---- 3. the fit ---------------------------------------------------------------------------------------------------------------------
def test_fit_recovers_f0_and_B_from_exact_tracks():
    rng = np.random.default_rng(5)
    T, K = 9, 14
    for base in (None, np.sort(rng.uniform(1.0, 12.0, K))):
        r = np.arange(1, K + 1, dtype=np.float64) if base is None else base
        f0 = rng.uniform(80.0, 400.0, (2, T, 1))
        Bc = np.array([2.5e-4, 0.0])
        f = f0 * (r * np.sqrt(1.0 + Bc[:, None, None] * r * r))
        weight = rng.uniform(0.1, 1.0, (2, T, K))
        weight[1, 3] = 0.0                                                               # a frame without weight keeps the f0 given
        given = rng.uniform(80.0, 400.0, (2, T, 1))
        got0, gotB = ddsp.fit_inharmonicity(t64(f), t64(weight), base_ratios=None if base is None else t64(base), f0=t64(given))
        assert got0.dtype == torch.float64 and got0.shape == (2, T, 1) and gotB.shape == (2,)
        live = np.ones((2, T), dtype=bool)
        live[1, 3] = False
        err0 = np.abs(got0.numpy()[..., 0] / f0[..., 0] - 1.0)[live].max()
        print(f"exact tracks ({'integers' if base is None else 'other ratios'}): f0 off by {err0:.2e}, B by {np.abs(gotB.numpy() - Bc).max():.2e}")
        # y spans 1 .. 1 + B K^2 while B is read from its slope: the fit's condition number is a few K^2
        assert err0 <= 64 * K * K * EPS64 and np.abs(gotB.numpy() - Bc).max() <= 64 * K * K * EPS64
        assert got0.numpy()[1, 3, 0] == given[1, 3, 0]
    # compressed partials: the line's slope is negative, B is clamped at 0 and f0 is the scale of the plain series
    r = np.arange(1, K + 1, dtype=np.float64)
    f = 100.0 * r * np.sqrt(1.0 - 1e-4 * r * r)
    got0, gotB = ddsp.fit_inharmonicity(t64(np.tile(f, (1, 3, 1))), torch.ones(1, 3, K, dtype=torch.float64))
    assert float(gotB[0]) == 0.0 and np.allclose(got0.numpy(), (r * f).sum() / (r * r).sum(), rtol=1e-14)
    none0, noneB = ddsp.fit_inharmonicity(torch.zeros(1, 2, 3), torch.ones(1, 2, 3))
    assert not none0.any() and float(noneB[0]) == 0.0                                     # nothing usable: zeros, no NaN


# ---- 4. the harmonic analysis is the special case -----------------------------------------------------------------------------------
def test_equals_the_harmonic_analysis_on_exact_multiples():
    """f0 a multiple of 1/8 Hz keeps k f0 exact in fp32 (and so in fp64): the two analyses see the same tracks.  The harmonic one
    takes theta as a running fp64 sum over the N samples and multiplies by k, this one the closed form: the phases differ by at most
    (N + T + 8) 2^-53 (|P| + 1) turns; the rest of the tolerance is test 1's."""
    B, T, hop, Wn, K = 2, 16, 32, 128, 6
    rng = np.random.default_rng(9)
    f0 = (np.round(rng.uniform(150.0, 400.0, (B, T, 1)) * 8) / 8).astype(np.float32).astype(np.float64)
    f = f0 * np.arange(1, K + 1)
    assert np.array_equal(f, (f0.astype(np.float32) * np.arange(1, K + 1, dtype=np.float32)).astype(np.float64))
    audio = rng.standard_normal((B, T * hop))
    voiced = torch.ones(B, T, 1, dtype=torch.bool)
    voiced[0, 5] = False
    got = ddsp.partial_analysis(t64(audio), t64(f), hop, SR, Wn, voiced=voiced, return_complex=True)
    want = ddsp.harmonic_analysis(t64(audio), t64(f0), hop, SR, K, Wn, voiced=voiced, return_complex=True)
    pmax = max(np.abs(pr.phases(f[b], hop, SR, cast=False)).max() for b in range(B))
    gain = 2.0 * np.abs(audio).max()                                                     # (2 / norm) sum |w x| <= 2 max |x|
    tol = np.sqrt(2.0) * gain * (2 * np.pi * (T * hop + T + 8) * EPS64 * (pmax + 1.0) + (Wn + 16) * EPS64)
    err = (got["C"] - want["C"]).abs().max().item()
    print(f"partial_analysis against harmonic_analysis on k f0: {err:.2e} (tolerance {tol:.2e})")
    assert err <= tol and (got["a"] - want["a"]).abs().max().item() <= K * tol
    assert torch.equal(got["C"] == 0, want["C"] == 0)


# ---- 5. masks and hygiene -----------------------------------------------------------------------------------------------------------
def test_masks_zero_exactly_their_own_entries():
    B, T, hop, Wn, K = 1, 10, 16, 64, 4
    rng = np.random.default_rng(3)
    audio = t64(rng.standard_normal((B, T * hop)))
    f = np.tile(np.array([300.0, 700.0, 1900.0, 3100.0]), (B, T, 1))
    clean = ddsp.partial_analysis(audio, t64(f), hop, SR, Wn, return_complex=True)
    bad = f.copy()
    bad[0, 2, 0], bad[0, 3, 1], bad[0, 4, 2], bad[0, 5, 3] = np.nan, -5.0, 0.0, SR // 2 + 1.0
    voiced = torch.ones(B, T, 1, dtype=torch.bool)
    voiced[0, 7] = False
    got = ddsp.partial_analysis(audio, t64(bad), hop, SR, Wn, voiced=voiced, return_complex=True)
    dead = np.zeros((T, K), dtype=bool)
    dead[2, 0] = dead[3, 1] = dead[4, 2] = dead[5, 3] = True
    dead[7] = True
    assert np.array_equal(got["C"][0].numpy() == 0, dead) and torch.isfinite(got["a"]).all() and torch.isfinite(got["c"]).all()
    assert np.array_equal(got["f"][0].numpy(), np.where(pr.usable(bad[0]), bad[0], 0.0))
    silent = ddsp.partial_analysis(audio, torch.zeros(B, T, K, dtype=torch.float64), hop, SR, Wn)
    assert not silent["a"].any() and torch.equal(silent["c"], torch.full((B, T, K), 1.0 / K, dtype=torch.float64))
    # a NaN sample reaches only the frames whose windows hold it
    at = 5 * hop + 3
    poisoned = audio.clone()
    poisoned[0, at] = np.nan
    nan = ddsp.partial_analysis(poisoned, t64(f), hop, SR, Wn, return_complex=True, reassign=True)
    holds = np.array([ref.frame_start(t, hop, Wn) <= at < ref.frame_start(t, hop, Wn) + Wn for t in range(T)])
    assert holds.sum() == Wn // hop
    assert torch.isnan(nan["a"][0, holds, 0]).all() and torch.equal(nan["C"][0, ~holds], clean["C"][0, ~holds])
    assert torch.equal(nan["f_re"][0, holds], t64(f)[0, holds])                          # not measurable: the entry itself
    harm = ddsp.partial_resynthesis(clean["C"], t64(f), hop, SR)
    assert harm.shape == (B, T * hop) and torch.isfinite(harm).all()


def test_refusals_and_the_empty_batch():
    audio, f = torch.zeros(2, 64), torch.full((2, 4, 3), 440.0)
    with pytest.raises(RuntimeError, match="no backward"):
        ddsp.partial_analysis(audio.clone().requires_grad_(), f, 16, SR, 32)
    with pytest.raises(RuntimeError, match="no backward"):
        ddsp.partial_analysis(audio, f.clone().requires_grad_(), 16, SR, 32)
    with pytest.raises(RuntimeError, match="no backward"):
        ddsp.refine_partials(audio, f.clone().requires_grad_(), 16, SR, 32)
    with pytest.raises(ValueError, match="samples"):
        ddsp.partial_analysis(audio[:, :60], f, 16, SR, 32)
    with pytest.raises(ValueError, match="even"):
        ddsp.partial_analysis(audio, f, 16, SR, 33)
    with pytest.raises(ValueError, match="voiced"):
        ddsp.partial_analysis(audio, f, 16, SR, 32, voiced=torch.ones(2, 4))
    with pytest.raises(ValueError, match="model"):
        ddsp.inharmonic_analysis(audio, f[..., :1], 16, SR, 3, 32, model='loose')
    with pytest.raises(ValueError, match="max_cents"):
        ddsp.refine_partials(audio, f, 16, SR, 32, max_cents=0.0)
    with pytest.raises(ValueError, match="complex"):
        ddsp.partial_resynthesis(torch.zeros(2, 4, 3), f, 16, SR)
    empty = ddsp.partial_analysis(audio[:0], f[:0], 16, SR, 32, return_complex=True, reassign=True)
    assert empty["C"].shape == (0, 4, 3) and empty["a"].shape == (0, 4, 1) and empty["f_re"].shape == (0, 4, 3)
    harm, resid, _ = ddsp.partial_residual(audio[:0], f[:0], 16, SR, 32)
    assert harm.shape == resid.shape == (0, 64) and ddsp.refine_partials(audio[:0], f[:0], 16, SR, 32).shape == (0, 4, 3)
    d = ddsp.inharmonic_analysis(audio[:0], f[:0, :, :1], 16, SR, 3, 32)
    assert d["ratios"].shape == (0, 4, 3) and d["inharmonicity"].shape == (0,)
    half = ddsp.partial_analysis(audio.half(), f, 16, SR, 32)                            # 16-bit floats: analysed in fp32
    assert half["a"].dtype == torch.float32


# ---- 6. wiring ----------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("ddsp_partials_supported", "ddsp_partials_workspace_bytes", "ddsp_partials_analysis", "ddsp_partials_resynth")


def test_exports_and_symbols():
    for name in ("partials", "PartialAnalyzer", "partial_analysis", "partial_resynthesis", "partial_residual", "refine_partials",
                 "fit_inharmonicity", "inharmonic_analysis"):
        assert name in ddsp.__all__ and hasattr(ddsp, name), name
    header = open(os.path.join(ROOT, "include", "ddsp_hip.h")).read()
    names = list(ddsp._lib.SIGNATURES)
    lib = ddsp._lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\(", header), name                             # declared
        assert name in ddsp._lib.EXPORTS and getattr(lib, name).argtypes is not None, name          # exported and bound
    at = names.index("ddsp_sinusoids_set_grid")
    assert tuple(names[at + 1:at + 5]) == NEW_SYMBOLS                                    # directly after the ddsp_sinusoids_* entries
    assert lib.ddsp_hip_abi_version() == 5 == ddsp._lib.ABI_VERSION
    assert "#define DDSP_PARTIALS_PHASE_READY 1u" in header and ddsp.partials.PHASE_READY == 1


def test_entry_points_validate_before_any_device_access():
    lib = ddsp._lib.lib()
    buffer = ctypes.create_string_buffer(64)                         # (a valid address; nothing is read from it)
    p = (ctypes.addressof(buffer) + 15) & ~15
    ok = dict(B=1, T=4, K=8, hop=16, W=64, sr=SR)

    def analysis(ptr, **kw):
        s = dict(ok, **kw)
        return lib.ddsp_partials_analysis(ptr, ptr, None, ptr, ptr, ptr, None, ptr, s["B"], s["T"], s["K"], s["hop"], s["W"], s["sr"], None)

    def resynth(ptr, flags=0, **kw):
        s = dict(ok, **kw)
        return lib.ddsp_partials_resynth(ptr, ptr, None, ptr, None, ptr, s["B"], s["T"], s["K"], s["hop"], s["sr"], flags, None)

    for call in (analysis, resynth):
        assert call(None) == -1 and call(None, B=0) == 0                                # null pointers; the empty batch before them
        assert call(None, B=-1) == -1 and call(p, T=0) == -1 and call(p, K=0) == -1 and call(p, hop=0) == -1 and call(p, sr=0) == -1
        assert call(None, K=257) == -1                                                   # null pointers before the range
        assert call(p, K=257) == -2 and call(p, hop=1025) == -2 and call(p, T=(1 << 20) + 1, hop=16) == -2
        assert call(p, B=1 << 38, T=4) == -2
    assert analysis(p, W=63) == -1 and analysis(p, W=0) == -1 and analysis(p, W=4098) == -2
    assert resynth(p, flags=2) == -1 and resynth(p + 4) == -1                            # an unknown flag; C not 8-byte aligned
    sup = lib.ddsp_partials_supported
    assert sup(256, 1024, 4096) == 1 and sup(1, 1, 2) == 1
    assert sup(257, 64, 256) == 0 and sup(0, 64, 256) == 0 and sup(8, 1025, 256) == 0 and sup(8, 0, 256) == 0
    assert sup(8, 64, 4098) == 0 and sup(8, 64, 0) == 0 and sup(8, 64, 255) == 0
    size = lib.ddsp_partials_workspace_bytes
    tracks = 3 * 8 * 2 * 10 * 7
    assert 2 * 4 * 4096 + tracks <= size(2, 10, 7, 16, 64) <= 2 * 4 * 4096 + tracks + 3 * 256
    assert size(0, 10, 7, 16, 64) == 0 and size(2, 10, 257, 16, 64) == 0 and size(2, 10, 7, 16, 63) == 0
    assert size(2, (1 << 20) + 1, 7, 16, 64) == 0


def test_autoencoder_and_bank_wiring():
    from encoder_common import AEConf
    x = torch.zeros(1, 4096)
    for synth in ("harmonic", "wavetable"):
        with pytest.raises(ValueError, match="inharmonic"):
            ddsp.AutoEncoder(AEConf, tracker="yin", synth=synth).analyse_partials(x)
    ae = ddsp.AutoEncoder(AEConf, tracker="yin", synth="inharmonic")
    with pytest.raises(ValueError, match="inharmonic"):
        ae.analyse(x)                                                                    # as before
    with pytest.raises(ValueError, match="noise must be"):
        ae.analyse_partials(x, noise="pink")
    with pytest.raises(ValueError, match="overlap"):
        ae.analyse_partials(x, noise="overlap_add")
    with pytest.raises(ValueError, match="model"):
        ae.analyse_partials(x, model="loose")

    bank = ae.decoder.harmonics
    keys = list(bank.state_dict())
    K, T = bank.n_partials, 6
    rho = pr.stretched(K, 2e-4)
    detune = np.linspace(-4.0, 5.0, K)
    ratios = np.tile(rho * 2.0 ** (detune / 1200.0), (2, T, 1))
    c = np.random.default_rng(1).uniform(0.1, 1.0, (2, T, K))
    ctrl = dict(f0=torch.full((2, T, 1), 200.0), ratios=torch.from_numpy(ratios).float(), a=torch.ones(2, T, 1),
                c=torch.from_numpy(c).float(), inharmonicity=torch.tensor([1e-4, 3e-4]))
    bank.init_from(ctrl)
    assert abs(float(bank.inharmonicity.detach()) - 2e-4) < 1e-9 and list(bank.state_dict()) == keys
    assert np.abs(bank.detune_cents.detach().numpy() - detune).max() < 1e-3              # (ratios were rounded to fp32: 2e-4 cents)
    assert bank.inharmonicity.requires_grad and bank.detune_cents.requires_grad
    ctrl["c"][:, :, 3] = 0.0
    bank.init_from(ctrl)
    assert float(bank.detune_cents.detach()[3]) == 0.0                                   # a partial without weight keeps detune 0

    an = ddsp.PartialAnalyzer(AEConf, iterations=1)
    assert not list(an.parameters()) and an.n_partials == AEConf.n_harmonics and an.win_length == AEConf.n_fft
    Tn = 8
    y = torch.randn(1, Tn * AEConf.hop_length, dtype=torch.float64)
    d = an(y, torch.full((1, Tn, 1), 100.0, dtype=torch.float64))
    assert d["ratios"].shape == (1, Tn, AEConf.n_harmonics) and torch.isfinite(d["a"]).all()


# ---- 7. the device bounds mean something ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", pr.GPU_SHAPES)
def test_bounds_are_tight_enough_to_mean_something_at_every_gpu_case(shape):
    B, T, hop, Wn, K, sr = shape
    audio, f, voiced = pr.string_rows(*shape)
    inter = pr.interior_frames(T, hop, Wn)
    for b in range(B):
        want = pr.analyse(audio[b], f[b], hop, sr, Wn, voiced[b])
        _, bound_h = pr.resynth(want["C"], f[b], hop, sr)
        top = np.abs(want["C"]).max()
        assert 0 < want["bound_C"].max() <= 1e-2 * top
        assert want["bound_a"].max() <= 1e-2 * want["a"].max()
        assert np.isfinite(want["bound_c"]).any() and want["bound_c"][np.isfinite(want["bound_c"])].max() <= 1e-2 * want["c"].max()
        assert bound_h.max() <= 1e-2 * top
        if inter:
            held = np.isfinite(want["bound_f"])
            assert want["vacuous"] == 0                                                  # the 10^-3 rule is the only one that leaves entries out
            assert want["bound_Du"].max() <= 1e-2 * np.abs(want["Du"]).max()
            assert held.any() and want["bound_f"][held].max() <= 1e-2 * np.abs(want["f_re"][held]).max()
