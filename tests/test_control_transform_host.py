"""The control transformation without a GPU: the definition's own behaviour
(tests/control_transform_reference.py, fp64), the package's CPU fp64 path against it, the argument checks, the entry point's
binding, and the bound the device tests use.  Every test prints its observed maximum before it asserts.

TOL_A, the bound on |A'_device - A'_fp64| relative to the largest amplitude A of the output frame's two source rows (and on
|N'_device - N'_fp64| relative to the largest band of the two rows).  The kernel differs from the definition only by its fp32
arithmetic: S as an fp32 wavefront sum, a / S and c (a / S) rounded, mu and nu rounded to fp32, the two convex combinations with
every product and sum rounded, a' as an fp32 wavefront sum and c' = A' / a' rounded (the tests read A' back as a' c').  The frame
map (i0, i1, lambda), u, v, f0' and every mask are exact or fp64 in both.  reference.transform_fp32 is that arithmetic operation
by operation, in the kernel's own summation order; test_device_bound evaluates it on the device tests' own inputs and finds
1.64e-7 for A' and 1.04e-7 for N'.  TOL_A = 4e-7 is twice the larger figure (another order of the same sums is as valid),
rounded up, and stays far below the project's audio contract of 1e-5."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ddsp_pytorch_amd as ddsp
import control_transform_reference as ref

EINVAL, ERANGE = -1, -2
SR = ref.SAMPLE_RATE
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def controls(f0, a, c, noise=None, dtype=torch.float64):
    """One row or a batch of numpy controls -> the package's dict in `dtype`."""
    f0, a, c = (np.asarray(v) for v in (f0, a, c))
    if f0.ndim == 1:
        f0, a, c, noise = f0[None], a[None], c[None], None if noise is None else np.asarray(noise)[None]
    out = dict(f0=torch.from_numpy(f0).to(dtype)[..., None], a=torch.from_numpy(a).to(dtype)[..., None], c=torch.from_numpy(c).to(dtype))
    if noise is not None:
        out["H"] = torch.from_numpy(np.asarray(noise)).to(dtype)
    return out


def definition(f0, a, c, noise, T_out=None, stretch=1.0, transpose=0.0, formant=0.0, pos=None, H_out=None):
    """The definition of one row with the package's scalar conventions."""
    pos = ref.stretch_positions(len(f0), stretch) if pos is None else np.asarray(pos, np.float32)
    r = np.broadcast_to(ref.ratio_of(transpose), pos.shape)
    q = r if formant is None else np.broadcast_to(ref.ratio_of(formant), pos.shape)
    return ref.transform(f0, a, c, noise, pos, r, q, SR, c.shape[-1] if H_out is None else H_out)


def small_row(T=12, H=20, F=9, f0=50.0, seed=3):
    rng = np.random.default_rng(seed)
    return (np.full(T, f0, dtype=np.float32), rng.uniform(0.1, 1.0, T).astype(np.float32),
            rng.uniform(0.05, 1.0, (T, H)).astype(np.float32), rng.uniform(0.0, 1.0, (T, F)).astype(np.float32))


@pytest.mark.parametrize("shape", ref.GPU_SHAPES)
def test_cpu_path_matches_the_definition_in_fp64(shape):
    B, T, T_out, H, H_out, F = shape
    x = ref.rows(shape)
    out = ddsp.transform_controls(controls(x["f0"], x["a"], x["c"], x["N"]), SR, transpose=torch.from_numpy(x["transpose"]),
                                  formant=torch.from_numpy(x["formant"])[..., None], positions=torch.from_numpy(x["pos"]), n_harmonics=H_out)
    assert sorted(out) == ["H", "a", "c", "f0"] and all(v.dtype == torch.float64 for v in out.values())
    assert out["f0"].shape == out["a"].shape == (B, T_out, 1) and out["c"].shape == (B, T_out, H_out) and out["H"].shape == (B, T_out, F)
    r, q = ref.ratio_of(x["transpose"]), ref.ratio_of(x["formant"])
    worst = 0.0
    for b in range(B):
        w = ref.transform(x["f0"][b], x["a"][b], x["c"][b], x["N"][b], x["pos"][b], r[b], q[b], SR, H_out)
        assert np.array_equal(out["f0"][b, :, 0].numpy(), w["f0"].astype(np.float64)), b
        worst = max(worst, np.abs(out["a"][b, :, 0].numpy() - w["a"]).max(), np.abs(out["c"][b].numpy() - w["c"]).max(),
                    np.abs(out["H"][b].numpy() - w["N"]).max())
    print(f"{shape}: CPU fp64 path against the definition, max difference {worst:.3e}")
    assert worst <= 1e-10


def test_cpu_path_keeps_fp32_and_the_module_is_the_function():
    shape = B, T, T_out, H, H_out, F = ref.GPU_SHAPES[2]
    x = ref.rows(shape)
    kw = dict(transpose=torch.from_numpy(x["transpose"]), formant=torch.from_numpy(x["formant"]), positions=torch.from_numpy(x["pos"]))
    ctrl = controls(x["f0"], x["a"], x["c"], x["N"], dtype=torch.float32)
    ctrl["hidden"] = torch.zeros(3)                              # keys that are no controls are dropped
    out = ddsp.transform_controls(ctrl, SR, **kw)
    assert sorted(out) == ["H", "a", "c", "f0"] and all(v.dtype == torch.float32 for v in out.values())
    r, q = ref.ratio_of(x["transpose"]), ref.ratio_of(x["formant"])
    worst = 0.0
    for b in range(B):
        w = ref.transform(x["f0"][b], x["a"][b], x["c"][b], x["N"][b], x["pos"][b], r[b], q[b], SR, H_out)
        A = (out["a"][b] * out["c"][b]).double().numpy() * (w["a"] != 0)[:, None]
        worst = max(worst, (np.abs(A - w["A"]) / np.maximum(w["scale"], 1e-30)[:, None]).max())
        assert np.array_equal(out["f0"][b, :, 0].numpy(), w["f0"])
    print(f"CPU fp32 path against the definition: {worst:.3e} of the largest source amplitude")
    assert worst <= 1e-5                                         # torch's own order of H = 100 fp32 terms; the audio contract
    module = ddsp.ControlTransform(type("Conf", (), dict(sample_rate=SR)))
    assert not list(module.parameters()) and isinstance(module, torch.nn.Module)
    again = module(ctrl, **kw)
    assert all(torch.equal(out[k], again[k]) for k in out)
    assert ddsp.transform_controls is ddsp.analysis.transform_controls and "transform_controls" in ddsp.__all__ and "ControlTransform" in ddsp.__all__


def test_identity():
    shape = B, T, _, H, _, F = (2, 16, 16, 180, 180, 195)
    x = ref.rows(shape)
    out = ddsp.transform_controls(controls(x["f0"], x["a"], x["c"], x["N"]), SR, stretch=1, transpose=0, formant=0)
    worst = 0.0
    for b in range(B):
        w = definition(x["f0"][b], x["a"][b], x["c"][b], x["N"][b])
        A = ref.source_amplitudes(x["f0"][b], x["a"][b], x["c"][b], SR)
        voiced = ref.voiced_of(x["f0"][b])
        assert voiced.any() and not voiced.all()
        for f0_out in (w["f0"], out["f0"][b, :, 0].numpy().astype(np.float32)):
            assert np.array_equal(f0_out[voiced].view(np.uint32), x["f0"][b][voiced].view(np.uint32))
            # (an unvoiced frame in front of a voiced one takes that one's f0, at amplitude 0; inside a run f0' = 0)
            assert not f0_out[~voiced & ~np.append(voiced[1:], voiced[-1])].any()
        worst = max(worst, np.abs(w["a"][:, None] * w["c"] * (w["a"] != 0)[:, None] - A).max(),
                    np.abs((out["a"][b] * out["c"][b]).numpy() * (w["a"] != 0)[:, None] - A).max())
        assert np.array_equal(w["N"], x["N"][b].astype(np.float64)) and np.array_equal(out["H"][b].numpy(), w["N"])
    print(f"identity: max |a' c' - A| = {worst:.3e}")
    assert worst <= 1e-12


def test_formants_stay_where_they_are():
    """An envelope that is linear in Hz is reproduced by linear interpolation: after +7 semitones with the formants kept every
    audible harmonic sits on the same line; the slack is the fp32 rounding of c."""
    T, H, f0 = 4, 40, 200.0
    line = lambda f: np.maximum(0.0, 1.0 - f / 9000.0)                                           # noqa: E731
    c = np.tile(line(f0 * np.arange(1, H + 1)), (T, 1))
    c = (c / c.sum(-1, keepdims=True)).astype(np.float32)
    row = (np.full(T, f0, dtype=np.float32), np.full(T, 0.8, dtype=np.float32), c, None)
    A = ref.source_amplitudes(*row[:3], SR)
    w = definition(*row, transpose=7.0, formant=0.0)
    audible = ~w["masked"][0]
    freq = w["u"][0] * f0                                        # k' f0', exactly
    want = A[0, 0] / line(f0) * line(freq)
    err = np.abs(w["A"][0][audible] / want[audible] - 1.0).max()
    print(f"+7 semitones, formants kept: {audible.sum()} audible harmonics, max relative error {err:.3e}")
    assert audible.sum() == 26 and (freq[audible] <= 8000).all()
    assert err <= 1e-7
    assert not w["A"][0][w["u"][0] > H].any() and (w["u"][0] > H).any()                            # above the source's top harmonic
    follow = definition(*row, transpose=7.0, formant=None)
    assert np.array_equal(follow["A"][0][audible], A[0][audible]) and not follow["A"][0][~audible].any()
    # the package agrees (fp64 path)
    out = ddsp.transform_controls(controls(*row[:3]), SR, transpose=7.0, formant=0.0)
    assert np.abs((out["a"][0] * out["c"][0]).numpy() - w["A"]).max() <= 1e-12
    out = ddsp.transform_controls(controls(*row[:3]), SR, transpose=7.0, formant=None)
    assert np.abs((out["a"][0] * out["c"][0]).numpy() - follow["A"]).max() <= 1e-12


def test_down_an_octave_holds_below_the_fundamental():
    row = small_row(f0=400.0)
    A = ref.source_amplitudes(*row[:3], SR)
    w = definition(*row, transpose=-12.0, formant=0.0)
    assert np.array_equal(w["f0"], np.full(12, 200.0, dtype=np.float32))
    assert np.array_equal(w["A"][:, 0], A[:, 0]) and np.array_equal(w["A"][:, 1], A[:, 0])
    assert np.array_equal(w["A"][:, 2], (A[:, 0] + A[:, 1]) / 2)


def test_formant_shift_alone():
    T, H, F = 12, 20, 9
    row = small_row(T, H, F, f0=50.0)
    A, N = ref.source_amplitudes(*row[:3], SR), row[3].astype(np.float64)
    up = definition(*row, formant=12.0, H_out=2 * H + 4)
    assert np.array_equal(up["f0"], row[0])
    assert np.array_equal(up["A"][:, 1:2 * H:2], A) and not up["A"][:, 2 * H:].any()              # A'[2 m] = A[m], zeros above 2 H
    assert np.array_equal(up["N"][:, ::2], N[:, :(F + 1) // 2])                                   # N'[2 j] = N[j]
    down = definition(*row, formant=-12.0)
    assert np.array_equal(down["N"][:, :(F + 1) // 2], N[:, ::2]) and not down["N"][:, (F + 1) // 2:].any()   # zeros above
    assert np.array_equal(down["A"][:, :H // 2], A[:, 1::2]) and not down["A"][:, H // 2:].any()
    out = ddsp.transform_controls(controls(*row), SR, formant=12.0, n_harmonics=2 * H + 4)
    assert np.abs((out["a"][0] * out["c"][0]).numpy() - up["A"]).max() <= 1e-12 and np.array_equal(out["H"][0].numpy(), up["N"])


def test_stretch():
    T, H, F = 12, 20, 9
    f0, a, c, N = small_row(T, H, F, f0=300.0)
    a = np.linspace(0.1, 1.2, T).astype(np.float32)                                              # a linear ramp
    c = np.tile(c[0], (T, 1))
    for s in (0.3, 0.75, 1.0, 1.5, 2.0, 2.46):
        out = ddsp.transform_controls(controls(f0, a, c, N), SR, stretch=s)
        T_out = max(1, int(np.floor(T * s + 0.5)))
        assert out["f0"].shape == (1, T_out, 1) and out["c"].shape == (1, T_out, H) and out["H"].shape == (1, T_out, F), s
        pos = ref.stretch_positions(T, s)
        assert len(pos) == T_out and pos.min() >= 0 and pos.max() <= T - 1
        w = definition(f0, a, c, N, stretch=s)
        assert np.abs(out["a"][0, :, 0].numpy() - w["a"]).max() <= 1e-12
    w = definition(f0, a, c, N, stretch=2.0)
    A = ref.source_amplitudes(f0, a, c, SR)
    assert np.array_equal(w["A"][0], A[0]) and np.array_equal(w["A"][-1], A[-1])                  # the ends are the input's ends
    assert np.array_equal(w["N"][0], N[0].astype(np.float64)) and np.array_equal(w["N"][-1], N[-1].astype(np.float64))
    pos = ref.stretch_positions(T, 2.0).astype(np.float64)
    ramp = np.interp(pos, np.arange(T), a.astype(np.float64))
    err = np.abs(w["a"] - ramp).max()
    print(f"stretch 2 on a ramp of a: max |a' - ramp(pos)| = {err:.3e}")
    assert err <= 1e-12
    # a voiced / unvoiced boundary, and runs of unvoiced frames
    f0 = np.full(T, 300.0, dtype=np.float32)
    f0[4:8] = (0.0, np.nan, -1.0, np.inf)
    w = definition(f0, a, c, N, stretch=3.0)
    assert set(np.unique(w["f0"])) == {np.float32(0.0), np.float32(300.0)}                        # never a glide from 0
    pos = ref.stretch_positions(T, 3.0).astype(np.float64)
    fade = (pos > 3) & (pos < 4)
    assert fade.sum() >= 2 and (w["f0"][fade] == 300.0).all()
    assert (np.diff(w["a"][fade]) < 0).all() and (w["a"][fade] > 0).all() and (w["a"][fade] < A[3].sum()).all()
    inside = (pos >= 4) & (pos < 7)                               # both neighbours unvoiced
    assert inside.sum() >= 6 and not w["f0"][inside].any() and not w["a"][inside].any() and (w["c"][inside] == 1.0 / H).all()
    out = ddsp.transform_controls(controls(f0, a, c, N), SR, stretch=3.0)
    assert np.array_equal(out["f0"][0, :, 0].numpy(), w["f0"].astype(np.float64)) and np.abs(out["c"][0].numpy() - w["c"]).max() <= 1e-12
    # a time map: reversed, and frozen on one frame
    back = ddsp.transform_controls(controls(f0, a, c, N), SR, positions=torch.arange(T - 1, -1, -1.0))
    same = ddsp.transform_controls(controls(f0, a, c, N), SR)
    assert torch.equal(back["a"], same["a"].flip(1)) and torch.equal(back["H"], same["H"].flip(1))
    still = ddsp.transform_controls(controls(f0, a, c, N), SR, positions=torch.full((1, 5), 2.0))
    assert torch.equal(still["c"], same["c"][:, 2:3].expand(-1, 5, -1)) and still["a"].shape == (1, 5, 1)


def test_output_nyquist():
    T, H = 6, 20
    f0, a, c, _ = small_row(T, H, f0=300.0)                      # 20 x 300 = 6000 Hz: every source harmonic is audible
    w = definition(f0, a, c, None, transpose=12.0, formant=None)
    k = np.arange(1, H + 1)
    gone = k * 600.0 > 8000
    assert gone.sum() == 7 and np.array_equal(w["masked"][0], gone)
    assert not w["A"][:, gone].any() and (w["A"][:, ~gone] > 0).all()                             # exactly those
    assert np.abs(w["c"].sum(-1) - 1.0).max() <= 1e-12 and not w["c"][:, gone].any()
    out = ddsp.transform_controls(controls(f0, a, c), SR, transpose=12.0, formant=None)
    assert np.array_equal(out["c"][0].numpy() == 0, np.tile(gone, (T, 1))) and np.abs(out["c"][0].numpy().sum(-1) - 1.0).max() <= 1e-12


def test_hostile_per_frame_values_on_the_cpu_path():
    """NaN, infinite, zero and negative per-frame values follow the silent-frame and clamp rules (the device test's inputs)."""
    T, H, F = 6, 8, 5
    f0, a, c, N = small_row(T, H, F, f0=100.0)
    f0[1], f0[4] = np.nan, np.inf
    bad = np.array([np.nan, np.inf, -np.inf, 0.0, -3.0, 1e30, 2.5, 2.5, 2.5, 2.5, 2.5, 2.5], dtype=np.float32)
    semis = np.array([0, 0, 0, 0, 0, 0, np.nan, np.inf, -np.inf, 0, 0, 0], dtype=np.float32)
    form = np.array([0, 0, 0, 0, 0, 0, 0, 0, 0, np.nan, np.inf, -np.inf], dtype=np.float32)
    out = ddsp.transform_controls(controls(f0, a, c, N), SR, positions=torch.from_numpy(bad), transpose=torch.from_numpy(semis),
                                  formant=torch.from_numpy(form))
    w = ref.transform(f0, a, c, N, bad, ref.ratio_of(semis), ref.ratio_of(form), SR, H)
    assert all(torch.isfinite(v).all() for v in out.values())
    assert np.array_equal(w["i0"][:6], [0, T - 1, 0, 0, 0, T - 1])                                # the clamp; a NaN counts as 0
    assert np.array_equal(w["ok"], [True] * 6 + [False] * 6)
    silent = ~w["live"]
    assert silent[6:].all() and not out["f0"][0, silent].any() and not out["a"][0, silent].any()
    assert (out["c"][0, silent] == 1.0 / H).all() and not out["H"][0, 6:].any()
    assert np.array_equal(out["f0"][0, :, 0].numpy(), w["f0"].astype(np.float64)) and np.abs(out["c"][0].numpy() - w["c"]).max() <= 1e-12
    assert np.abs(out["H"][0].numpy() - w["N"]).max() <= 1e-12


def test_argument_checks():
    f0, a, c, N = small_row()
    good = controls(f0, a, c, N)
    call = lambda ctrl=good, **kw: ddsp.transform_controls(ctrl, SR, **kw)                         # noqa: E731
    for key, value in (("f0", good["f0"][..., 0]), ("a", good["a"][:, :-1]), ("c", good["c"][:, :-1]), ("c", good["c"][0]),
                       ("H", good["H"][:, 1:]), ("f0", good["f0"].to("meta")), ("H", good["H"].to("meta"))):
        with pytest.raises(ValueError):                          # shapes, and a tensor on another device
            call(dict(good, **{key: value}))
    with pytest.raises(ValueError):
        call({k: v for k, v in good.items() if k != "a"})
    for s in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            call(stretch=s)
    for kw in (dict(transpose=float("nan")), dict(formant=float("inf")), dict(transpose=1e6), dict(n_harmonics=0)):
        with pytest.raises(ValueError):
            call(**kw)
    with pytest.raises(ValueError):                              # positions replaces stretch
        call(positions=torch.zeros(4), stretch=2.0)
    with pytest.raises(ValueError):
        call(positions=torch.zeros(2, 4))                        # another batch
    with pytest.raises(ValueError):
        call(positions=torch.zeros(4), transpose=torch.zeros(5))
    with pytest.raises(ValueError):
        call(transpose=torch.zeros(12, device="meta"))
    with pytest.raises(ValueError):
        call(transpose=torch.zeros(5))                           # T' = 12 from the stretch
    for key in ("f0", "a", "c", "H"):                            # no backward: refused as the analysis refuses it
        with pytest.raises((ValueError, RuntimeError)):
            call(dict(good, **{key: good[key].clone().requires_grad_()}))
    with pytest.raises((ValueError, RuntimeError)):
        call(transpose=torch.zeros(12, requires_grad=True))
    empty = call({k: v[:0] for k, v in good.items()}, stretch=1.5, n_harmonics=7)
    assert empty["f0"].shape == empty["a"].shape == (0, 18, 1) and empty["c"].shape == (0, 18, 7) and empty["H"].shape == (0, 18, 9)
    assert sorted(call({k: v for k, v in good.items() if k != "H"})) == ["a", "c", "f0"]


def test_symbol_is_bound_and_the_abi_is_still_5():
    text = open(os.path.join(ROOT, "include", "ddsp_hip.h")).read()
    assert re.search(r"\bint\s+ddsp_transform_controls\s*\(", text)
    order = list(ddsp._lib.EXPORTS)
    assert order[order.index("ddsp_noise_analysis_ola") + 1] == "ddsp_transform_controls"         # the table keeps the header's order
    L = ddsp._lib.lib()
    assert L.ddsp_hip_abi_version() == 5 == ddsp._lib.ABI_VERSION
    assert L.ddsp_transform_controls.restype is ctypes.c_int
    assert list(L.ddsp_transform_controls.argtypes) == ([ctypes.c_void_p] * 11 + [ctypes.c_long] * 3 + [ctypes.c_int] * 4 + [ctypes.c_void_p])


def test_entry_point_checks_return_before_any_launch():
    """Every call here is refused (or is the empty batch) by the host checks: the pointers are never dereferenced."""
    L = ddsp._lib.lib()
    p, N = 4096, None                                            # a non-null address that is never read
    def call(ptrs, B=2, T=16, T_out=24, H=20, H_out=20, F=65, sr=16000):
        return L.ddsp_transform_controls(*ptrs, B, T, T_out, H, H_out, F, sr, N)
    good = (p,) * 11
    bare = (p, p, p, N, p, p, p, p, p, p, N)                     # no noise in, none out
    assert call((N,) * 11, B=0) == 0
    for i in (0, 1, 2, 4, 5, 6, 7, 8, 9):
        assert call(tuple(N if k == i else v for k, v in enumerate(good))) == EINVAL, i
        assert call(tuple(N if k == i else v for k, v in enumerate(bare))) == EINVAL, i
    assert call(tuple(N if k == 3 else v for k, v in enumerate(good))) == EINVAL                  # noise without noise_out,
    assert call(tuple(N if k == 10 else v for k, v in enumerate(good))) == EINVAL                 # and the reverse
    for kw in (dict(B=-1), dict(T=0), dict(T_out=0), dict(H=0), dict(H_out=0), dict(F=0), dict(sr=0), dict(T=-4), dict(H_out=-1)):
        assert call(good, **kw) == EINVAL and call(bare, **kw) == EINVAL, kw
    for kw in (dict(H=257), dict(H_out=257), dict(F=258), dict(B=1 << 30, T=1 << 30), dict(B=1 << 30, T_out=1 << 30),
               dict(B=1 << 40, T=1 << 40)):
        assert call(good, **kw) == ERANGE and call(bare, **kw) == ERANGE, kw
    # the order: pointers and signs before ranges
    assert call((N,) * 11, H=257) == EINVAL and call(good, H=257, T=0) == EINVAL


def test_device_bound():
    """TOL_A from the kernel's arithmetic on the device tests' own inputs (see the module's docstring)."""
    fig_a = fig_n = 0.0
    reached = dict(below=0, above=0, one_voiced=0, masked=0, audible=0)
    for shape in ref.GPU_SHAPES:
        B, T, T_out, H, H_out, F = shape
        x = ref.rows(shape)
        r, q = ref.ratio_of(x["transpose"]), ref.ratio_of(x["formant"])
        for b in range(B):
            args = (x["f0"][b], x["a"][b], x["c"][b], x["N"][b], x["pos"][b], r[b], q[b], SR, H_out)
            w, g = ref.transform(*args), ref.transform_fp32(*args)
            assert np.array_equal(g["f0"].view(np.uint32), w["f0"].view(np.uint32))
            A = g["a"].astype(np.float64)[:, None] * g["c"].astype(np.float64) * (g["a"] != 0)[:, None]
            assert np.array_equal(A == 0, w["A"] == 0) and np.array_equal(g["N"] == 0, w["N"] == 0)
            loud, hiss = w["scale"] > 0, w["nscale"] > 0
            ea = (np.abs(A - w["A"])[loud] / w["scale"][loud, None]).max() if loud.any() else 0.0
            en = (np.abs(g["N"] - w["N"])[hiss] / w["nscale"][hiss, None]).max() if hiss.any() else 0.0
            print(f"{shape} row {b}: fp32 arithmetic, A' {ea:.3e}, N' {en:.3e} of the largest source value")
            fig_a, fig_n = max(fig_a, ea), max(fig_n, en)
            u = w["u"][w["live"]]
            reached["below"] += int((u < 1).sum())
            reached["above"] += int((u > H).sum())
            reached["one_voiced"] += int((w["ok"] & (w["va"] != w["vb"])).sum())
            reached["masked"] += int(w["masked"][w["live"]].sum())
            reached["audible"] += int((~w["masked"][w["live"]]).sum())
    print(f"derived bound: 2 x max({fig_a:.3e}, {fig_n:.3e}) = {2 * max(fig_a, fig_n):.3e}; TOL_A = {ref.TOL_A:g}; branches {reached}")
    assert all(reached.values())
    assert 2 * max(fig_a, fig_n) <= ref.TOL_A <= 1e-5
    assert ref.TOL_A <= 1.5 * 2 * max(fig_a, fig_n)                                              # twice the figure, rounded up: no more
