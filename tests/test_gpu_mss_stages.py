"""One scale of the spectral loss (csrc/ddsp_mss_fft.hip: mss_wave_kernel<64..1024>, mss_wave2048_kernel; the fp64 finish of
ddsp_mss.hip), the gather behind it (ddsp_stft_frames_backward) and the per-bin pass of the library-FFT path (ddsp_spectral_loss)
through direct ctypes calls, no autograd, against the fp64 reference and the derived bounds of tests/mss_reference.py: every bin
of every frame of the gradient spectrum (recovered from the device's gradient frames by an fp64 rfft), the two terms on their
own, the walk over more units than the grid, quiet frames beside loud ones inside normalised audio, which frames a non-finite
sample reaches, and what is written where.  Every test prints the figures it asserts on (`pytest -s`).

The two terms each meet 2e-5 of the reference on every case here (worst measured figures are printed per case as `worst term
error / 2e-05`); the fallback to CPU_FACTOR times the stock fp32 formulation's error is only taken by a term that misses it."""
import numpy as np
import pytest

import mss_reference as M

pytestmark = pytest.mark.gpu

U = M.U


def show(lines):
    for line in lines:
        print(line)


# ---- a. every bin of every frame, b. the three outputs ----------------------------------------------------------------------
@pytest.mark.parametrize("alpha,eps", M.ALPHA_EPS)
@pytest.mark.parametrize("n", M.SIZES)
def test_every_bin_of_every_frame(n, alpha, eps):
    """Per shape of M.GPU_SHAPES: every bin under check_bins, lin and log under check_terms, out3[0] their rounded sum, no NaN
    left, the guard untouched, the same out3 bits without grad_frames, the cap on undecided bins; the identical row exactly zero
    (frames, and lin and log when it is launched alone); a repeat bit-identical; a row the same bits wherever it stands in the
    batch (the count, and with it the rounded 1 / count, differs between B = 1 and B = 3, so `alone` means: alone in its pairs
    and units, the other rows exchanged and permuted) and, launched as B = 1, the same gradient frames times 3 to rounding."""
    lines, ok, worst = [], True, 0.0
    for shape in M.GPU_SHAPES:
        if shape[1] != n:
            continue
        name, _, hop, B, L = shape
        xp, xt = M.shape_inputs(shape)
        good, w, r, fr = M.run_case(xp, xt, n, hop, alpha, eps, name, lines)
        ok &= good
        worst = max(worst, w)
        fr2, o3 = M.device_scale(xp, xt, n, hop, alpha, eps)
        ok &= np.array_equal(M.bits(fr2), M.bits(fr))
        if B == 3:
            ok &= bool(np.all(M.bits(fr[2]) << 1 == 0))                           # +-0: sign(0) = 0 and P - Q = 0 in bits
            _, o_same = M.device_scale(xp[2:], xt[2:], n, hop, alpha, eps)
            ok &= float(o_same[0]) == 0.0 and float(o_same[1]) == 0.0 and float(o_same[2]) == 0.0
            # row 0 third in another batch: other neighbours, another slot of its unit, another turn of the pipeline
            other_p, other_t = M.signals(n + hop, 2, L)
            fr3, _ = M.device_scale(np.concatenate([other_p, xp[:1]]), np.concatenate([other_t, xt[:1]]), n, hop, alpha, eps)
            ok &= np.array_equal(M.bits(fr3[2]), M.bits(fr[0]))
            fr1, _ = M.device_scale(xp[:1], xt[:1], n, hop, alpha, eps)
            # (1 / count rounds differently: 2 U on the spectrum, then two transforms' worth of different roundings)
            tol = 2.0 * (M.transform_ceiling(n) + 4.0 * U) * M.pair_norm(np.linalg.norm(fr[0].astype(np.float64), axis=-1), n)
            ok &= bool(np.all(np.linalg.norm(fr1[0].astype(np.float64) / 3.0 - fr[0], axis=-1) <= tol))
        if not ok:
            lines.append(f"MSS {name}: FAILED (first failing shape of this size)")
            break
    show(lines)
    print(f"MSS every bin n{n} alpha {alpha} eps {eps}: worst error / bound {worst:.4f}")
    assert ok


def test_one_unit_and_the_whole_grid_go_through_the_finish_kernel():
    """blocks = 1 (one unit: B = 1, two frames at n_fft 1024) and blocks = 4096 (the beyond-the-grid cases below) both sum their
    partials in the fp64 finish; here the one-unit end, and B = 0 (no launch: three zeros)."""
    xp, xt = M.signals(5, 1, 1024 // 2 + 1 + 400)
    lines = []
    ok, _, r, fr = M.run_case(xp, xt, 1024, 1024, 1.0, 1e-7, "one unit", lines)
    show(lines)
    assert ok and fr.shape[1] == 1 and M.units(1024, 1, 1) == 1
    fr0, o3 = M.device_scale(np.zeros((0, 600)), np.zeros((0, 600)), 1024, 256, 1.0, 1e-7)
    assert fr0.size == 0 and np.all(M.bits(o3) == 0)


def test_the_scale_entry_refuses_an_eps_below_the_normal_range():
    xp, xt = M.signals(6, 1, 100)
    for eps in (1.1754942e-38, 1e-40, 0.0):
        M.device_scale(xp, xt, 64, 16, 1.0, eps, expect=M.EINVAL)
    M.device_scale(xp, xt, 64, 16, 1.0, 1.1754944e-38)


# ---- c. more units than the grid --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", M.BEYOND, ids=[s[0] for s in M.BEYOND])
def test_more_units_than_the_grid(shape):
    """More than 4096 units from small signals (the entry takes any hop > 0): between 4096 and 8192 some wavefronts walk two
    units and some one; above 8192 the software pipeline of the 64 .. 1024 kernel reaches its third stage with a ragged tail.
    Criteria (a) and (b) on every bin of every frame."""
    name, n, hop, B, L = shape
    xp, xt = M.signals(n + B, B, L)
    lines = []
    ok, worst, r, fr = M.run_case(xp, xt, n, hop, 1.0, 1e-7, name, lines)
    show(lines)
    print(f"MSS {name}: {M.units(n, B, 1 + L // hop)} units, worst error / bound {worst:.4f}")
    assert M.units(n, B, 1 + L // hop) > M.MAX_UNITS and ok


# ---- d. levels inside normalised audio --------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", M.LEVEL_SHAPES, ids=[s[0] for s in M.LEVEL_SHAPES])
def test_levels_inside_normalised_audio(shape):
    """|x| <= 1 with hop-long segments at levels 10^U(-4, 0) and a full-scale sine onset directly after a segment at 1e-4; hop =
    n_fft makes a pair a quiet and a loud disjoint frame.  The per-bin criterion holds with its dS relative to the pair (the
    kernel's design; the cap on undecided bins does not apply: beside a loud partner a quiet frame's bins are undecided by that
    rule).  Printed, not asserted: each frame's error relative to its OWN gradient spectrum's norm, by the partner / own ratio
    of the windowed frames' norms."""
    name, n, hop, B, L = shape
    xp, xt = M.level_inputs(shape)
    lines = []
    ok, worst, r, fr = M.run_case(xp, xt, n, hop, 1.0, 1e-7, name, lines, cap=False)
    show(lines)
    G = M.recover(fr)
    own = np.linalg.norm(G - r["G"], axis=-1) / np.linalg.norm(r["G"], axis=-1)
    level = np.linalg.norm(r["frames_p"], axis=-1)
    F = level.shape[1]
    partner = np.stack([np.where(np.arange(F) ^ 1 < F, row[np.minimum(np.arange(F) ^ 1, F - 1)], 0.0) for row in level])
    ratio = partner / level if n != 2048 else np.zeros_like(level)
    for lo, hi in ((0.0, 1.0), (1.0, 10.0), (10.0, 100.0), (100.0, np.inf)):
        sel = (ratio >= lo) & (ratio < hi)
        if sel.any():
            print(f"MSS {name}: partner / own level in [{lo:g}, {hi:g}): {int(sel.sum())} frames, worst own-relative error {own[sel].max():.2e}, median {np.median(own[sel]):.2e}")
    print(f"MSS {name}: worst error / bound {worst:.4f}")
    assert ok


# ---- e. non-finite containment ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", M.SIZES)
def test_a_non_finite_sample_reaches_only_the_frames_that_hold_it(n):
    """One NaN, then one Inf, in x_pred of row 1 of 3 -- inside the left mirror, mid-row, in the last n_fft / 2 samples -- and a
    NaN in x_true: only the frames whose reflect-padded window holds the sample, and below 2048 points their pair partners, may
    differ from the clean run; every other frame of every row is bit-identical to it and finite."""
    hop = n // 4
    B, L = 3, 13 * hop + 3
    F = 1 + L // hop
    xp, xt = M.signals(n + 9, B, L)
    clean, _ = M.device_scale(xp, xt, n, hop, 1.0, 1e-7)
    assert np.isfinite(clean).all()
    for where, pos in (("left mirror", 5), ("mid-row", L // 2 + 1), ("right mirror", L - 7)):
        for which, value in (("pred", np.nan), ("pred", np.inf), ("true", np.nan)):
            a, b = xp.copy(), xt.copy()
            (a if which == "pred" else b)[1, pos] = value
            got, _ = M.device_scale(a, b, n, hop, 1.0, 1e-7)
            hit = M.frames_holding(pos, n, hop, L)
            assert 0 < len(hit) < F
            keep = np.ones((B, F), dtype=bool)
            keep[1, hit] = False
            same = np.all(M.bits(got) == M.bits(clean), axis=-1)
            touched = sorted(set(np.nonzero(~same[1])[0]))
            print(f"MSS containment n{n} {where} {which} {value}: may differ {hit}, differ {touched}")
            assert same[keep].all(), (where, which, value, np.argwhere(~same & keep))
            assert np.isfinite(got[keep]).all()


# ---- f. the gather ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", M.SIZES)
def test_the_gather_alone(n):
    """ddsp_stft_frames_backward on the reference's fp32-rounded gradient frames against the fp64 gather within the summation
    bound of its ceil(n_fft / hop) + 2 terms; accumulate = 1 onto a random buffer is the fp32 sum of that buffer and the
    accumulate = 0 result, bit for bit.  Hops n_fft / 4, n_fft, 3 and L = n_fft / 2 + 1."""
    w = M.window_of(n)
    worst = 0.0
    for hop, B, L in ((n // 4, 3, 5 * (n // 4) + 3), (n // 4, 2, n // 2 + 1), (n, 2, 3 * n + 1), (3, 2, n // 2 + 1), (3, 1, n + 10)):
        xp, xt = M.signals(n + hop, B, L)
        r = M.scale(xp, xt, n, hop, 1.0, 1e-7)
        g32 = M.f32(r["grad_frames"])
        got = M.device_gather(g32, w, hop, L)
        ref = M.gather(g32, w, hop, L)
        bound = M.gather_bound(g32, w, hop, L)
        err = np.abs(got - ref)
        assert np.isfinite(got).all() and np.all(err <= bound), (hop, B, L, float((err / np.maximum(bound, 1e-300)).max()))
        worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
        buf = np.random.default_rng(n + L).standard_normal((B, L)).astype(np.float32)
        acc = M.device_gather(g32, w, hop, L, into=buf)
        assert np.array_equal(M.bits(acc), M.bits(buf + got))
        # against autograd's own answer: the gather of the exact frames is d loss / d x_pred
        assert np.abs(ref - M.gather(r["grad_frames"], w, hop, L)).max() <= 4.0 * U * np.abs(ref).max() * (-(-n // hop) + 2)
    print(f"MSS gather n{n}: worst error / summation bound {worst:.3f}")


# ---- g. ddsp_spectral_loss --------------------------------------------------------------------------------------------------
def _pass_case(nb, seed):
    """Spectra [nb] complex64: random bins over many decades; bins with P == Q in bits (pred == truth, pred == conj(truth)); bins
    with P = 0; bins at 1e-20 and 1e+15 in power."""
    rng = np.random.default_rng(seed)
    mag = 10.0 ** rng.uniform(-3.0, 2.0, nb)
    pred = (mag * np.exp(2j * np.pi * rng.random(nb))).astype(np.complex64)
    truth = (10.0 ** rng.uniform(-3.0, 2.0, nb) * np.exp(2j * np.pi * rng.random(nb))).astype(np.complex64)
    i = np.arange(nb)
    pred = np.where(i % 7 == 1, truth, pred)
    pred = np.where(i % 7 == 2, np.conj(truth), pred)
    pred = np.where(i % 11 == 3, 0.0, pred)
    truth = np.where(i % 13 == 4, 0.0, truth)
    pred = np.where(i % 17 == 5, pred / np.maximum(np.abs(pred), 1e-30) * 1e-10, pred)
    pred = np.where(i % 19 == 6, pred / np.maximum(np.abs(pred), 1e-30) * 10.0 ** 7.5, pred)
    return pred.astype(np.complex64), truth.astype(np.complex64)


@pytest.mark.parametrize("nb", [1, 255, 256, 257, 2048 * 256 + 1])
def test_the_per_bin_pass_of_the_library_fft_path(nb):
    """ddsp_spectral_loss: the spectra are the inputs, so dS = 0 and every bin's bound is coefficient_bound's count of the kernel's
    own steps (IEEE division: half an ulp); a bin with P == Q in bits has an exactly zero gradient; out3 under check_terms; the
    same three floats without the gradient.  eps from 1e-2 down to the smallest normal with every kind of bin, and a denormal eps
    on bins of nonzero power (1 / eps itself overflows fp32: with P = 0 no fp32 evaluation has a finite coefficient to multiply
    the zero spectrum with)."""
    for alpha, eps in ((1.0, 1e-7), (0.3, 1e-2), (1.0, 1.1754944e-38), (1.0, 1e-40)):
        pred, truth = _pass_case(nb, nb)
        eps = float(np.float32(eps))
        if eps < 1.1754944e-38:
            pred = np.where(pred == 0, np.complex64(1e-10), pred)
        S, T = pred.astype(np.complex128), truth.astype(np.complex128)
        P, Q = S.real ** 2 + S.imag ** 2, T.real ** 2 + T.imag ** 2
        a32 = float(np.float32(alpha))
        e = np.log2(Q + eps) - np.log2(P + eps)
        r = dict(lin=float(np.abs(P - Q).mean()), log=float(np.abs(e).mean()), alpha=alpha)
        g, o3 = M.device_spectral_loss(pred, truth, alpha, eps)
        _, o3n = M.device_spectral_loss(pred, truth, alpha, eps, want_grad=False)
        lines = []
        ok, _ = M.check_terms(r, o3, lines=lines, tag=f"pass nb {nb} eps {eps:g}")
        assert ok and np.array_equal(M.bits(o3), M.bits(o3n)), lines
        same = (pred == truth) | (pred == np.conj(truth))
        assert same.any() or nb < 7
        assert np.all(g[same] == 0) and np.isfinite(g.view(np.float32)).all()
        # a bin is undecided when the rounding of the powers and of the logs alone can turn a sign (dS = 0)
        dPQ = 3.0 * U * (P + Q)
        und = (np.abs(P - Q) <= 2.0 * dPQ + M.log_slack(P, Q, eps)) & ~same
        best = np.full(nb, np.inf)
        for sd in M.SIGNS:
            for se in M.SIGNS:
                c1 = np.where(und, M.coefficient(P, Q, a32, eps, sd, se), M.coefficient(P, Q, a32, eps))
                c1 = np.where(same, 0.0, c1)
                lim = (2.0 / nb) * M.coefficient_bound(np.abs(S), P, c1, 0.0, a32, eps, rcp_ulps=0.5)
                err = np.abs(g.astype(np.complex128) - (2.0 / nb) * c1 * S)
                with np.errstate(divide="ignore", invalid="ignore"):
                    best = np.minimum(best, np.where(lim > 0, err / lim, np.where(err == 0, 0.0, np.inf)))
        print(f"MSS pass nb {nb} alpha {alpha} eps {eps:g}: worst error / bound {best.max():.3f}, undecided {int(und.sum())}")
        assert best.max() <= 1.0, (int(np.argmax(best)), best.max())


def test_the_per_bin_pass_without_bins():
    g, o3 = M.device_spectral_loss(np.zeros(0, np.complex64), np.zeros(0, np.complex64), 1.0, 1e-7)
    assert np.all(M.bits(o3) == 0)
    M.device_spectral_loss(np.ones(4, np.complex64), np.ones(4, np.complex64), 1.0, 0.0, expect=M.EINVAL)
