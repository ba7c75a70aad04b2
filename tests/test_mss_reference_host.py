"""The fp64 reference and the bounds of tests/mss_reference.py checked on something this work did not write -- SpectralLoss in
fp64 on the CPU with autograd -- and by holding the stock fp32 formulation on the CPU to every bound on the inputs of the GPU
cases; the cap on undecided bins of every GPU case, from the reference alone.  All without a device."""
import numpy as np
import pytest
import torch

from ddsp_pytorch_amd.training import SpectralLoss

import mss_reference as M

U = M.U


def _hops(n):
    return (n // 4, n // 2, n // 8, n, 3, 1)


@pytest.mark.parametrize("n", M.SIZES)
def test_reference_equals_spectral_loss_in_fp64(n):
    """loss, lin, log and gather(grad_frames) == SpectralLoss(...).double() on the CPU (value and autograd's d loss / d x_pred) to
    1e-12 relative, for hops n/4, n/2, n/8, n, 3 and 1, at L = n/2 + 1 (both mirrors overlap) and a longer, ragged row; and
    recover(grad_frames) == G to 1e-12."""
    rng = np.random.default_rng(n)
    for hop in _hops(n):
        for B, L in ((2, n // 2 + 1), (1, min(2 * n + 7, n // 2 + 1 + 40 * hop))):
            for alpha, eps in ((1.0, 1e-7), (0.3, 1e-2)):
                xp, xt = 0.3 * rng.standard_normal((B, L)), 0.3 * rng.standard_normal((B, L))
                sl = SpectralLoss(n, alpha=alpha, eps=eps).double()
                sl.hop = hop
                w = sl.window.numpy()
                assert w.dtype == np.float64 and np.array_equal(w, w.astype(np.float32).astype(np.float64))
                tp = torch.from_numpy(xp).requires_grad_(True)
                tt = torch.from_numpy(xt)
                loss = sl(tp, tt)
                loss.backward()
                Pt, Qt = sl.power(tp.detach()), sl.power(tt)
                lin = float((Pt - Qt).abs().mean())
                log = float((torch.log2(Qt + eps) - torch.log2(Pt + eps)).abs().mean())
                r = M.scale(xp, xt, n, hop, alpha, eps, window=w)
                assert r["S"].shape == (B, 1 + L // hop, n // 2 + 1)
                assert np.abs(r["P"] - Pt.transpose(1, 2).numpy()).max() <= 1e-12 * float(Pt.max())
                for got, want in ((r["loss"], float(loss.detach())), (r["lin"], lin), (r["log"], log)):
                    assert abs(got - want) <= 1e-12 * abs(want), (hop, B, L, got, want)
                gx = M.gather(r["grad_frames"], w, hop, L)
                want = tp.grad.numpy()
                assert gx.shape == want.shape
                assert np.abs(gx - want).max() <= 1e-12 * np.abs(want).max(), (hop, B, L)
                Gr = M.recover(r["grad_frames"])
                assert np.abs(Gr - r["G"]).max() <= 1e-12 * np.abs(r["G"]).max()
                # the end bins are real: nothing is lost where the kernel keeps only their real parts
                assert np.abs(r["G"][..., 0].imag).max() <= 1e-12 * np.abs(r["G"]).max()
                assert np.abs(r["G"][..., -1].imag).max() <= 1e-12 * np.abs(r["G"]).max()


def test_shape_lists_reach_every_hazard():
    for n in M.SIZES:
        mine = [s for s in M.GPU_SHAPES if s[1] == n]
        Fs = {(s[2], s[3], 1 + s[4] // s[2]) for s in mine}
        assert {h for h, _, _ in Fs} >= {n // 4, n, 3, 1}
        assert any(B == 1 and F % 2 == 1 for _, B, F in Fs) and any(B == 3 and F % 2 == 0 for _, B, F in Fs)
        assert any(s[4] == n // 2 + 1 and (1 + s[4] // s[2]) % 2 == 0 and s[2] == 1 for s in mine)
        # a pair (a frame at 2048) wholly inside its row: the unpadded load
        inside = False
        for _, _, hop, B, L in mine:
            for f in range(0, 1 + L // hop, 2):
                start = f * hop - n // 2
                last = start + n + (hop if n != 2048 else 0)
                inside |= start >= 0 and last <= L and (n == 2048 or f + 1 < 1 + L // hop)
        assert inside, n
    got = {name: M.units(n, B, 1 + L // hop) for name, n, hop, B, L in M.BEYOND}
    assert got["n64_2turns"] == 4204 and got["n1024_2turns"] == 4267 and got["n2048_2turns"] == 4506
    for name, u in got.items():
        assert (M.MAX_UNITS < u < 2 * M.MAX_UNITS) if name.endswith("2turns") else (2 * M.MAX_UNITS < u < 3 * M.MAX_UNITS), (name, u)
    for name, n, hop, B, L in M.BEYOND:
        assert B * (1 + L // hop) * n * 4 < 100e6, name
    assert {s[1] for s in M.BEYOND if s[0].endswith("2turns")} == set(M.SIZES)


def _attainable(xp, xt, n, hop, alpha, eps, tag, cap):
    r = M.scale(xp, xt, n, hop, alpha, eps)
    Gs, lin, log = M.stock(xp, xt, n, hop, alpha, eps)
    lines = []
    ok, worst, share = M.check_bins(r, Gs, stock=None, lines=lines, tag=tag)          # the derived bound alone: no stock floor
    assert ok and worst <= 1.0, lines
    assert share <= M.UNDECIDED_CAP or not cap, lines
    return worst, share


@pytest.mark.parametrize("n", M.SIZES)
def test_bin_bound_is_attainable_and_the_cap_holds_on_the_gpu_cases(n):
    """The torch fp32 CPU formulation's per-bin error stays under bin_bound on the inputs of every case of the GPU module's
    every-bin test -- every bin, none excluded, undecided bins by the rule of check_bins -- and at most 0.5 % of a case's bins
    are undecided."""
    worst, top = 0.0, 0.0
    for shape in M.GPU_SHAPES:
        if shape[1] != n:
            continue
        xp, xt = M.shape_inputs(shape)
        for alpha, eps in M.ALPHA_EPS:
            w, s = _attainable(xp, xt, n, shape[2], alpha, eps, shape[0], cap=True)
            worst, top = max(worst, w), max(top, s)
    print(f"MSS host n{n}: stock fp32 worst error / bound {worst:.4f}, largest undecided share {100 * top:.3f} %")


@pytest.mark.parametrize("shape", M.LEVEL_SHAPES, ids=[s[0] for s in M.LEVEL_SHAPES])
def test_bin_bound_is_attainable_on_the_level_cases(shape):
    """Quiet frames beside loud ones: the bound is relative to the pair, and the stock formulation (which transforms every frame
    on its own) stays under it.  The share of undecided bins is printed, not capped: a quiet frame's bins beside a loud partner
    are undecided by design of the rule."""
    name, n, hop, B, L = shape
    xp, xt = M.level_inputs(shape)
    assert np.abs(xp).max() <= 1.0 and np.abs(xt).max() <= 1.0
    w, s = _attainable(xp, xt, n, hop, 1.0, 1e-7, name, cap=False)
    print(f"MSS host {name}: stock fp32 worst error / bound {w:.4f}, undecided share {100 * s:.3f} %")


@pytest.mark.parametrize("shape", M.BEYOND, ids=[s[0] for s in M.BEYOND])
def test_the_cap_holds_beyond_the_grid(shape):
    name, n, hop, B, L = shape
    xp, xt = M.signals(n + B, B, L)
    r = M.scale(xp, xt, n, hop, 1.0, 1e-7)
    share = float(M.undecided(r).mean())
    print(f"MSS host {name}: undecided share {100 * share:.3f} %")
    assert share <= M.UNDECIDED_CAP


def test_the_cap_holds_on_the_sweep():
    """The random cases of fuzz_parity.sweep_mss_stages for the seeds tests/test_gpu_fuzz.py runs."""
    for seed in M.SWEEP_SEEDS:
        rng = np.random.default_rng(seed)
        for _ in range(M.SWEEP_CASES):
            case = M.random_case(rng)
            xp, xt = M.case_inputs(case)
            r = M.scale(xp, xt, case["n_fft"], case["hop"], case["alpha"], case["eps"])
            assert float(M.undecided(r).mean()) <= M.UNDECIDED_CAP, case


def test_undecided_and_the_holding_frames():
    """A bin is undecided exactly inside the margin; an identical row is decided (sign 0); frames_holding counts the mirrors."""
    xp, xt = M.signals(3, 3, 200, zero_row=1, same_row=2)
    r = M.scale(xp, xt, 64, 16, 1.0, 1e-7)
    und = M.undecided(r)
    assert not und[2].any() and np.all(r["G"][2] == 0.0) and np.all(r["grad_frames"][2] == 0.0)
    dS, dT = M.spectrum_error(r["S"], 64), M.spectrum_error(r["T"], 64)
    assert np.all(dT[1] == 0.0) and np.all(dS > 0.0)
    margin = 2.0 * (M.power_error(np.abs(r["S"]), dS[..., None]) + M.power_error(np.abs(r["T"]), dT[..., None]))
    assert np.all(und[:2] >= (np.abs(r["P"] - r["Q"]) <= margin)[:2])
    assert M.frames_holding(0, 64, 16, 200) == [0, 1, 2, 3]                       # padded position 32 alone: frames 0 .. 2, partner 3
    assert M.frames_holding(5, 64, 16, 200, partners=False) == [0, 1, 2]          # 37 and its mirror 27
    assert M.frames_holding(199, 64, 16, 200, partners=False) == [11, 12]         # 231 only: the last sample has no mirror
    assert M.frames_holding(198, 64, 16, 200, partners=False) == [11, 12]         # 230 and its mirror 232
    assert M.frames_holding(100, 2048, 512, 3000) == [0, 1, 2]                    # 1124 and the mirror 924; no partners at 2048
