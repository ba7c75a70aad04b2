"""The fp64 reference and the bounds of tests/griffinlim_reference.py checked on their own -- against torch.istft / torch.stft in
fp64, and by holding the stock fp32 formulation on the CPU to every bound -- and the argument validation of the test hook
ddsp_griffinlim_stage.  All without a device (nothing here launches a kernel)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ddsp_pytorch_amd as ddsp

import griffinlim_reference as G

U = G.U


def _torch_window(shape):
    _, n, _, wl, *_ = shape
    return torch.ones(n, dtype=torch.float64) if wl == 0 else torch.from_numpy(G.f32(G.hann(wl)))


@pytest.mark.parametrize("shape", G.GPU_SHAPES, ids=[s[0] for s in G.GPU_SHAPES])
def test_reference_stages_equal_torch_in_fp64(shape):
    """synth + overlap == torch.istft (with `length`, win_length < n_fft, and zeros past the natural length); analysis ==
    torch.stft; the envelope == what istft divides by.  fp64 against fp64: 1e-12 of the largest value."""
    p = G.shape_setup(shape)
    n, hop, B, T, L = p["n_fft"], p["hop"], p["B"], p["T"], p["L"]
    w = _torch_window(shape)
    assert np.array_equal(G.f32(G.padded(w.numpy(), n)), p["window"])
    S, ang0, R, Rprev = G.random_state(5, B, T, n, 0.4)
    env = G.envelope(p["window"], hop, T, L)                               # (unrounded: torch's own is fp64 here)
    X = S * G.angles(R, Rprev, 0.4)
    kw = dict(n_fft=n, hop_length=hop, win_length=w.shape[0], window=w)
    want = torch.istft(torch.from_numpy(X).transpose(1, 2), length=L, **kw).numpy()
    fr = G.synth(S, p["window"], R=R, Rprev=Rprev, c=0.4)
    y = G.overlap(fr, env, hop, L)
    assert y.shape == want.shape == (B, L)
    assert np.abs(y - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    nat = G.natural_length(n, hop, T)
    assert np.all(y[:, nat:] == 0.0) and (L <= nat or shape[0] == "n64_rect_zero_tail")
    Rw = torch.stft(torch.from_numpy(y), center=True, pad_mode="reflect", onesided=True, return_complex=True, **kw).transpose(1, 2).numpy()
    Rg = G.analysis(y, p["window"], hop, T)
    assert Rg.shape == Rw.shape == (B, T, n // 2 + 1)
    assert np.abs(Rg - Rw).max() <= 1e-12 * max(1.0, np.abs(Rw).max())
    fr2, y2, R2 = G.step(S, p["window"], env, hop, L, R=R, Rprev=Rprev, c=0.4)
    assert np.array_equal(fr2, fr) and np.array_equal(y2, y) and np.array_equal(R2, Rg)
    # the initial-angle forms
    for a0 in (None, ang0):
        Xa = S * (1.0 if a0 is None else a0)
        want = torch.istft(torch.from_numpy(Xa + 0j).transpose(1, 2), length=L, **kw).numpy()
        got = G.overlap(G.synth(S, p["window"], ang0=a0), env, hop, L)
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


def test_shape_list_reaches_every_hazard():
    names = {s[0] for s in G.GPU_SHAPES}
    for n in G.SIZES:
        assert {f"n{n}_hann", f"n{n}_shortest"} <= names
        p = G.shape_setup(G.SHAPE_BY_NAME[f"n{n}_hann"])
        frames = p["B"] * p["T"]
        assert frames % 2 == 1 and p["T"] % 2 == 1 and p["B"] >= 2                 # a lone last frame; a pair across two rows
        assert frames % G.frames_per_unit(n) != 0 or n == 2048                     # a ragged last unit
        assert frames > G.frames_per_unit(n)                                       # more than one block
        q = G.shape_setup(G.SHAPE_BY_NAME[f"n{n}_shortest"])
        assert q["L"] == n // 2 + 1
        starts = q["hop"] * np.arange(q["T"]) - n // 2
        # every frame reflects at its start and every frame but the first (which ends at n_fft / 2 = L - 1) at its end as well ...
        assert np.all(starts < 0) and np.all(starts[1:] + n > q["L"])
        assert np.all(starts + n - 1 <= 2 * (q["L"] - 1))                          # ... once
        r = [s for s in G.GPU_SHAPES if s[1] == n and s[0].endswith("_ragged")]
        assert r and all(0 < s[3] < n and s[6] == s[2] - 1 for s in r)             # L = hop (T - 1) + hop - 1, win_length < n_fft
    a, b = G.shape_setup(G.SHAPE_BY_NAME["n2048_h512_L3072"]), G.shape_setup(G.SHAPE_BY_NAME["n2048_h512_L3071"])
    assert (a["L"], b["L"]) == (3072, 3071) and 4 * 512 - 1024 + 2048 == a["L"] and b["T"] > 4
    z = G.shape_setup(G.SHAPE_BY_NAME["n64_rect_zero_tail"])
    assert z["L"] - G.natural_length(64, 64, z["T"]) == 18 and np.all(z["window"] == 1.0)


def test_fp32_overlap_restatement_lies_within_the_summation_bound():
    for shape in G.GPU_SHAPES:
        p = G.shape_setup(shape)
        fr = G.f32(np.random.default_rng(3).standard_normal((p["B"], p["T"], p["n_fft"])))
        y32 = G.overlap_fp32(fr, p["env"], p["hop"], p["L"])
        assert y32.dtype == np.float32 and y32.shape == (p["B"], p["L"])
        ratio = np.abs(y32 - G.overlap(fr, p["env"], p["hop"], p["L"])) / np.maximum(G.overlap_bound(fr, p["env"], p["hop"], p["L"]), 1e-300)
        assert ratio.max() <= 1.0, (shape[0], ratio.max())
        assert ratio.max() >= 0.05 or G.covering(p["n_fft"], p["hop"]) == 1        # (not vacuous; one frame a sample and env 1: exact)
        assert np.all(y32[:, G.natural_length(p["n_fft"], p["hop"], p["T"]):] == 0.0)


def test_designed_inputs_keep_their_conditioning():
    for n in (64, 2048):
        S, R, Rprev, c, ill = G.designed_state(n, 2, 5, n)
        k = G.kappa(R, Rprev, c)
        assert c == float(np.float32(0.99 / 1.99))
        assert k.min() >= 1.0 and k[..., ~ill].max() <= 2.0 and (~ill).mean() >= 15.0 / 16.0
        assert k[..., ill].min() >= 64.0 and (n == 64 or 2.0e4 <= k[..., ill].max() <= 5.0e4)
        assert np.abs(R).min() >= 0.5 * (1 - U) and np.abs(R).max() <= 2.0 * (1 + U)
        # the premises of spec_bound's derivation
        assert np.all(np.abs(R) >= 0.15 * c * np.abs(Rprev)) and np.abs(R - c * Rprev).min() >= 2.0 ** -28


def _held(tag, err, bound):
    ratio = float(np.max(err / bound))
    print(f"GLREF {tag}: worst error / bound = {ratio:.3f}")
    assert ratio <= 1.0, (tag, ratio)
    return ratio


def _stock_within_bounds(tag, S, window, env, hop, L, **state):
    """The stock fp32 step against the fp64 step from the same fp32 inputs: every bound of the reference module holds."""
    n = window.shape[0]
    X = S * G.angles(state["R"], state.get("Rprev"), state.get("c", 0.0)) if state.get("R") is not None else G.spectrum(S, state.get("ang0"))
    Xs = G.stock_spectrum(S, **state).numpy().astype(np.complex128)
    bound = G.spec_bound(S, state.get("R"), state.get("Rprev"), state.get("c", 0.0))
    ok = bound > 0
    if state.get("R") is None:
        ok = ok & (np.arange(S.shape[-1]) % (n // 2) != 0)                        # (G.spectrum drops imaginary parts there)
    r_spec = _held(tag + " spectrum per bin", np.abs(Xs - X)[ok], bound[ok])
    fr, y, Rn = G.step(S, window, env, hop, L, **state)
    sf, sy, sR = G.stock_step(S, window, hop, L, **state)
    fb, yb, rb = G.step_bounds(S, window, env, hop, L, **state)
    _held(tag + " frames", G.frame_err(sf, fr), fb)
    _held(tag + " y", np.linalg.norm(sy - y, axis=1), yb)
    _held(tag + " R_next", G.frame_err(sR, Rn), rb)
    # each stage alone from exact inputs
    _held(tag + " analysis alone", G.frame_err(G.stock_analysis(G.f32(y), window, hop), G.analysis(G.f32(y), window, hop, S.shape[1])),
          G.analysis_ceiling(G.analysis(G.f32(y), window, hop, S.shape[1]), n))
    return r_spec


@pytest.mark.parametrize("case", G.G27)
def test_stock_fp32_step_is_within_every_bound_on_the_teacher_forced_g27_states(golden, case):
    """The bounds are attainable without the code under test.  Measured: the spectrum reaches 0.65 of its per-bin bound."""
    p = G.g27_setup(golden("g27_" + case))
    worst = 0.0
    for k, R, Rprev in G.teacher_forced_states(p):
        worst = max(worst, _stock_within_bounds(f"{case} k={k}", p["S"], p["window"], p["env"], p["hop"], p["L"], R=R, Rprev=Rprev, c=p["c"]))
    _stock_within_bounds(f"{case} k=0", p["S"], p["window"], p["env"], p["hop"], p["L"], ang0=p["ang0"])
    print(f"GLREF {case}: worst spectrum ratio over k = 1 .. 16: {worst:.3f}")


@pytest.mark.parametrize("n", [64, 512, 2048])
def test_stock_fp32_step_is_within_every_bound_on_the_designed_inputs(n):
    p = G.shape_setup(G.SHAPE_BY_NAME[f"n{n}_hann"])
    S, R, Rprev, c, _ = G.designed_state(n, p["B"], p["T"], n)
    _stock_within_bounds(f"designed n{n}", S, p["window"], p["env"], p["hop"], p["L"], R=R, Rprev=Rprev, c=c)
    ones = np.ones(n)
    _stock_within_bounds(f"designed n{n}, all-ones window", S, ones, G.f32(G.envelope(ones, n, p["T"], n * (p["T"] - 1))), n, n * (p["T"] - 1),
                         R=R, Rprev=Rprev, c=c)


# ---- the hook's argument checks (no launch: there is no device here) ---------------------------------------------------------
def _call(L, stage, S, ang0, R, Rprev, inp, window, env, out, B, T, n, hop, length, c):
    return L.ddsp_griffinlim_stage(stage, S, ang0, R, Rprev, inp, window, env, out, B, T, n, hop, length, c, None)


def test_stage_hook_validates_before_it_launches():
    L = ddsp._lib.lib()
    word = ctypes.c_uint64(0)                      # (a valid address; nothing is read from it)
    p = ctypes.addressof(word)
    N = None
    good = dict(B=2, T=5, n=64, hop=16, length=64, c=0.5)
    for stage in (G.SYNTH, G.OVERLAP, G.ANALYSIS):
        # a range error is reported only after every pointer the stage reads was there: ERANGE proves the pointer checks passed
        bad_T = dict(good, T=6)
        need = {G.SYNTH: ("S", "window"), G.OVERLAP: ("inp", "env"), G.ANALYSIS: ("inp", "window")}[stage]
        ptrs = dict(S=N, ang0=N, R=N, Rprev=N, inp=N, window=N, env=N, out=p)
        for name in need:
            ptrs[name] = p
        assert _call(L, stage, **ptrs, **bad_T) == G.ERANGE
        for name in need + ("out",):
            assert _call(L, stage, **dict(ptrs, **{name: N}), **bad_T) == G.EINVAL, (stage, name)
            assert _call(L, stage, **dict(ptrs, **{name: N}), **good) == G.EINVAL, (stage, name)
        everything = dict.fromkeys(ptrs, p)
        for k, v in (("B", 0), ("B", -1), ("T", 0), ("hop", 0), ("length", 0), ("c", -0.1), ("c", 1.0), ("c", float("nan"))):
            assert _call(L, stage, **everything, **dict(good, **{k: v})) == G.EINVAL, (stage, k, v)
        # ddsp_griffinlim's range checks
        for n in (32, 96, 1000, 4096):
            assert _call(L, stage, **everything, **dict(good, n=n)) == G.ERANGE, n
        assert _call(L, stage, **everything, **dict(good, T=4)) == G.ERANGE                     # 1 + L / hop != T
        assert _call(L, stage, **everything, **dict(good, length=32, T=3)) == G.ERANGE           # L <= n_fft / 2
        assert _call(L, stage, **everything, **dict(good, B=65536)) == G.ERANGE
        assert _call(L, stage, **everything, **dict(good, hop=1, length=1 << 24, T=(1 << 24) + 1)) == G.ERANGE
        assert _call(L, stage, **everything, **dict(good, B=65535, n=2048, hop=1, length=(1 << 24) - 1, T=1 << 24)) == G.ERANGE
    for stage in (-1, 3, 99):
        assert _call(L, stage, **dict.fromkeys(("S", "ang0", "R", "Rprev", "inp", "window", "env", "out"), p), **good) == G.EINVAL


def test_stage_hook_is_refused_without_opt_in():
    """DDSP_EPERM in a process that did not set DDSP_TEST_HOOKS=1 before the library was loaded, whatever the arguments (here:
    ones that an armed process answers with EINVAL / ERANGE, without a launch)."""
    code = ("import ctypes, sys; L = ctypes.CDLL(sys.argv[1]); w = ctypes.c_uint64(0); p = ctypes.c_void_p(ctypes.addressof(w)); "
            "v = ctypes.c_void_p; L.ddsp_griffinlim_stage.argtypes = [ctypes.c_int] + [v] * 8 + [ctypes.c_long, ctypes.c_long, "
            "ctypes.c_int, ctypes.c_int, ctypes.c_long, ctypes.c_float, v]; "
            "print(L.ddsp_test_hooks_enabled(), *[L.ddsp_griffinlim_stage(s, p, p, p, p, p, p, p, p, 2, 6, 64, 16, 64, 0.5, None) "
            "for s in (0, 1, 2, 7)], L.ddsp_griffinlim_stage(0, None, p, p, p, p, p, p, p, 2, 5, 64, 16, 64, 0.5, None))")
    env = {k: v for k, v in os.environ.items() if k != "DDSP_TEST_HOOKS"}
    out = subprocess.run([sys.executable, "-c", code, ddsp._lib.SO_PATH], env=env, capture_output=True, text=True, check=True).stdout.split()
    assert out == ["0"] + ["-3"] * 5, out
    env["DDSP_TEST_HOOKS"] = "1"
    out = subprocess.run([sys.executable, "-c", code, ddsp._lib.SO_PATH], env=env, capture_output=True, text=True, check=True).stdout.split()
    assert out == ["1", "-2", "-2", "-2", "-1", "-1"], out
