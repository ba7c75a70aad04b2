"""The control morph without a GPU: the definition's own behaviour (tests/control_morph_reference.py,
fp64), the package's CPU path against it, the argument checks, the entry point's binding, and the bound the device tests use.
Every test prints its observed maximum before it asserts.

TOL_M, the bound on |A'_device - A'_fp64| relative to the largest amplitude A of the output frame's four source rows (and on
|N'_device - N'_fp64| relative to the largest band of the four rows).  The kernel differs from the definition only by its fp32
arithmetic: per sound S as an fp32 wavefront sum, a / S and c (a / S) rounded, mu rounded to fp32, the convex combinations across
harmonics, across frames and across the sounds with every product and sum rounded, a' as an fp32 wavefront sum and c' = A' / a'
rounded (the tests read A' back as a' c').  The frame maps, the weights, u_X and every mask are exact or fp64 in both, and f0' is
handed to the definition (teacher forcing; it is held to one fp32 ulp on its own).  reference.morph_fp32 is that arithmetic
operation by operation, in the kernel's own summation order; test_device_bound evaluates it on the device tests' own inputs and
finds 1.40e-7 for A' and 1.46e-7 for N'.  TOL_M = 3e-7 is twice the larger figure (another order of the same sums is as valid),
rounded up, and stays far below the project's audio contract of 1e-5."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ddsp_pytorch_amd as ddsp
import control_morph_reference as ref
import control_transform_reference as tref

EINVAL, ERANGE = -1, -2
SR = ref.SAMPLE_RATE
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(shape, coordinates) for shape in ref.GPU_SHAPES for coordinates in ref.COORDINATES]


def controls(x, dtype=torch.float64, noise=True):
    """A sound of the reference (one row or a batch of numpy arrays) -> the package's dict in `dtype`."""
    f0, a, c = (np.asarray(x[k]) for k in ("f0", "a", "c"))
    N = x.get("N") if noise else None
    if f0.ndim == 1:
        f0, a, c, N = f0[None], a[None], c[None], None if N is None else np.asarray(N)[None]
    out = dict(f0=torch.from_numpy(f0).to(dtype)[..., None], a=torch.from_numpy(a).to(dtype)[..., None], c=torch.from_numpy(c).to(dtype))
    if N is not None:
        out["H"] = torch.from_numpy(np.asarray(N)).to(dtype)
    return out


def package(x, H_out, coordinates, dtype=torch.float64):
    """morph_controls on the batch x of ref.rows, every per-frame argument given."""
    t = torch.from_numpy
    return ddsp.morph_controls(controls(x["a"], dtype), controls(x["b"], dtype), SR, mix_f0=t(x["wf"]), mix_harmonics=t(x["wh"])[..., None],
                               mix_noise=t(x["wn"]), coordinates=coordinates, positions_a=t(x["a"]["pos"]), positions_b=t(x["b"]["pos"]),
                               n_harmonics=H_out)


def ulps(x, y):
    """The distance of two arrays of non-negative fp32 values in units in the last place."""
    return np.abs(np.asarray(x, np.float32).view(np.int32).astype(np.int64) - np.asarray(y, np.float32).view(np.int32).astype(np.int64))


def check_f0(f0, w, where=""):
    """f0' of a path against the definition's: the same bits where it is selected, within one ulp where it went through exp2 / log2."""
    f0 = np.asarray(f0, np.float32)
    d = ulps(f0, w["f0_definition"])
    assert not d[w["selected"]].any(), where
    assert d.max() <= 1, where
    return int(d.max())


def sound(f0, a, c, N=None, pos=None):
    out = dict(f0=np.asarray(f0, np.float32), a=np.asarray(a, np.float32), c=np.asarray(c, np.float32))
    if N is not None:
        out["N"] = np.asarray(N, np.float32)
    if pos is not None:
        out["pos"] = np.asarray(pos, np.float32)
    return out


def small_sound(T=12, H=20, F=9, f0=50.0, seed=3):
    rng = np.random.default_rng(seed)
    return sound(np.full(T, f0), rng.uniform(0.1, 1.0, T), rng.uniform(0.05, 1.0, (T, H)), rng.uniform(0.0, 1.0, (T, F)))


def definition(xa, xb, T_out=None, mix=0.5, mix_f0=None, mix_harmonics=None, mix_noise=None, coordinates="hz", H_out=None, f0=None):
    """The definition of one row with the package's scalar conventions (linear maps onto T', None: T_a)."""
    T_out = len(xa["f0"]) if T_out is None else T_out
    xa = dict(xa, pos=xa.get("pos", ref.linear_positions(len(xa["f0"]), T_out)))
    xb = dict(xb, pos=xb.get("pos", ref.linear_positions(len(xb["f0"]), T_out)))
    w = [np.broadcast_to(np.asarray(mix if v is None else v, np.float32), (T_out,)) for v in (mix_f0, mix_harmonics, mix_noise)]
    H_out = max(xa["c"].shape[-1], xb["c"].shape[-1]) if H_out is None else H_out
    return ref.morph(xa, xb, *w, SR, H_out, coordinates, f0=f0)


def amplitudes(out, b=0):
    """a' c' of row b of the package's answer, 0 on the frames whose c' is the fill."""
    a, c = out["a"][b].double().numpy(), out["c"][b].double().numpy()
    return a * c * (a != 0)


@pytest.mark.parametrize("shape,coordinates", CASES)
def test_cpu_path_matches_the_definition_in_fp64(shape, coordinates):
    B, T_a, T_b, T_out, H_a, H_b, H_out, F = shape
    x = ref.rows(shape)
    out = package(x, H_out, coordinates)
    assert sorted(out) == ["H", "a", "c", "f0"] and all(v.dtype == torch.float64 for v in out.values())
    assert out["f0"].shape == out["a"].shape == (B, T_out, 1) and out["c"].shape == (B, T_out, H_out) and out["H"].shape == (B, T_out, F)
    worst = off = 0
    for b in range(B):
        f0 = out["f0"][b, :, 0].numpy().astype(np.float32)
        assert np.array_equal(f0.astype(np.float64), out["f0"][b, :, 0].numpy())                   # fp32 values whatever the dtype
        w = ref.morph(*ref.row_of(x, b), SR, H_out, coordinates, f0=f0)
        off = max(off, check_f0(f0, w, (shape, b)))
        worst = max(worst, np.abs(out["a"][b, :, 0].numpy() - w["a"]).max(), np.abs(out["c"][b].numpy() - w["c"]).max(),
                    np.abs(out["H"][b].numpy() - w["N"]).max())
    print(f"{shape} {coordinates}: CPU fp64 path against the definition, max difference {worst:.3e}; f0' within {off} ulp")
    assert worst <= 1e-10


def test_cpu_path_keeps_fp32_and_the_module_is_the_function():
    shape = B, T_a, T_b, T_out, H_a, H_b, H_out, F = ref.GPU_SHAPES[2]
    x = ref.rows(shape)
    t = torch.from_numpy
    kw = dict(mix_f0=t(x["wf"]), mix_harmonics=t(x["wh"]), mix_noise=t(x["wn"]), positions_a=t(x["a"]["pos"]), positions_b=t(x["b"]["pos"]))
    ctrl_a, ctrl_b = controls(x["a"], torch.float32), controls(x["b"], torch.float32)
    ctrl_a["hidden"] = torch.zeros(3)                            # keys that are no controls are dropped
    out = ddsp.morph_controls(ctrl_a, ctrl_b, SR, **kw)
    assert sorted(out) == ["H", "a", "c", "f0"] and all(v.dtype == torch.float32 for v in out.values())
    assert out["c"].shape == (B, T_out, max(H_a, H_b))
    worst = 0.0
    for b in range(B):
        f0 = out["f0"][b, :, 0].numpy()
        w = ref.morph(*ref.row_of(x, b), SR, max(H_a, H_b), "hz", f0=f0)
        check_f0(f0, w)
        worst = max(worst, (np.abs(amplitudes(out, b) - w["A"]) / np.maximum(w["scale"], 1e-30)[:, None]).max())
    print(f"CPU fp32 path against the definition: {worst:.3e} of the largest source amplitude")
    assert worst <= 1e-5                                         # torch's own order of H = 100 fp32 terms; the audio contract
    module = ddsp.ControlMorph(type("Conf", (), dict(sample_rate=SR)))
    assert not list(module.parameters()) and isinstance(module, torch.nn.Module)
    again = module(ctrl_a, ctrl_b, **kw)
    assert all(torch.equal(out[k], again[k]) for k in out)
    assert ddsp.morph_controls is ddsp.analysis.morph_controls and "morph_controls" in ddsp.__all__ and "ControlMorph" in ddsp.__all__


@pytest.mark.parametrize("coordinates", ref.COORDINATES)
def test_mix_0_and_1_are_the_transformation_of_one_sound(coordinates):
    """a', c' and the bands are transform_controls' on every frame; f0' on every frame where that sound is present (where it is
    absent and the other present, f0' is the other's pitch at amplitude 0: the definition's rule for one sound present)."""
    shape = B, T_a, T_b, T_out, H_a, H_b, H_out, F = ref.GPU_SHAPES[2]
    x = ref.rows(shape)
    pos = {k: torch.from_numpy(x[k]["pos"]) for k in "ab"}
    seen = 0
    for mix, key in ((0.0, "a"), (1.0, "b")):
        out = ddsp.morph_controls(controls(x["a"]), controls(x["b"]), SR, mix=mix, coordinates=coordinates, positions_a=pos["a"],
                                  positions_b=pos["b"], n_harmonics=H_out)
        want = ddsp.transform_controls(controls(x[key]), SR, positions=pos[key], n_harmonics=H_out)
        assert all(torch.equal(out[k], want[k]) for k in ("a", "c", "H")), (mix, key)
        present = torch.from_numpy(np.stack([ref.source_map(x[key]["f0"][b], x[key]["pos"][b])["present"] for b in range(B)]))
        assert torch.equal(out["f0"][present], want["f0"][present]) and not want["f0"][~present].any()
        assert not out["a"][~present].any()
        seen += int(present.sum()) * int((~present).sum() > 0)
        w = ref.morph(*ref.row_of(x, 0)[:2], *(np.full(T_out, mix, np.float32),) * 3, SR, H_out, coordinates)
        t = tref.transform(x[key]["f0"][0], x[key]["a"][0], x[key]["c"][0], x[key]["N"][0], x[key]["pos"][0], np.ones(T_out, np.float32),
                           np.ones(T_out, np.float32), SR, H_out)
        assert np.array_equal(w["A"], t["A"]) and np.array_equal(w["N"], t["N"])                    # the two definitions, in fp64
    assert seen


def test_the_same_pitch_gives_the_same_answer_in_both_coordinates():
    xa, xb = small_sound(12, 20, 9, f0=310.0, seed=3), small_sound(9, 26, 9, f0=310.0, seed=4)
    mix = torch.linspace(0.0, 1.0, 12)
    out = [ddsp.morph_controls(controls(xa), controls(xb), SR, mix=mix, coordinates=c) for c in ref.COORDINATES]
    assert all(torch.equal(out[0][k], out[1][k]) for k in out[0]) and float(out[0]["a"].min()) > 0
    assert (out[0]["f0"] == 310.0).all()                         # exp2(log2 f) is kept within [f, f]
    w = [definition(xa, xb, mix=mix.numpy(), coordinates=c) for c in ref.COORDINATES]
    assert np.array_equal(w[0]["A"], w[1]["A"]) and np.array_equal(w[0]["ua"], w[1]["ua"])


def test_formants_stay_where_they_are_in_hz_coordinates():
    """Two sounds a fifth apart under one envelope that is linear in Hz: in 'hz' coordinates any pitch weight with any amplitude
    weight returns that line at the new harmonics, wherever both sounds define it (at and above both fundamentals, up to the
    lower of their top audible harmonics); the slack is the fp32 rounding of c.  In 'harmonic' coordinates it does not."""
    T, H, fa, fb, gain = 4, 40, 200.0, 300.0, 0.02
    line = lambda f: np.maximum(0.0, 1.0 - f / 9000.0)                                           # noqa: E731
    sounds = []
    for f0 in (fa, fb):
        hz = f0 * np.arange(1, H + 1)
        env = line(hz)
        c = np.tile(env / env.sum(), (T, 1))
        sounds.append(sound(np.full(T, f0), np.full(T, gain * env[hz <= SR // 2].sum()), c))
    top = min(fa * H, fb * np.floor(SR / 2 / fb))                 # 7800 Hz: B's harmonic 26
    worst, apart = 0.0, 0.0
    for wf, wh in ((0.0, 0.3), (0.25, 0.0), (0.5, 0.5), (0.8, 1.0), (1.0, 0.6)):
        w = definition(*sounds, mix_f0=wf, mix_harmonics=wh, coordinates="hz")
        hz = np.arange(1, H + 1) * float(w["f0"][0])
        inside = (hz >= max(fa, fb)) & (hz <= top)
        assert inside.sum() >= 20
        worst = max(worst, np.abs(w["A"][0][inside] / (gain * line(hz[inside])) - 1.0).max())
        out = ddsp.morph_controls(controls(sounds[0]), controls(sounds[1]), SR, mix_f0=wf, mix_harmonics=wh)
        assert np.abs(amplitudes(out) - w["A"]).max() <= 1e-12 and check_f0(out["f0"][0, :, 0].numpy(), w) <= 1
        h = definition(*sounds, mix_f0=wf, mix_harmonics=wh, coordinates="harmonic")
        if 0 < wh < 1:
            apart = max(apart, np.abs(h["A"][0][inside] / (gain * line(hz[inside])) - 1.0).max())
    print(f"a fifth apart, one line over Hz: 'hz' within {worst:.3e} of the line, 'harmonic' up to {apart:.3f} off it")
    assert worst <= 1e-6 and apart > 0.05


def test_pitch_is_interpolated_in_log_frequency():
    xa, xb = small_sound(6, 8, 5, f0=200.0), small_sound(6, 8, 5, f0=400.0, seed=5)
    out = ddsp.morph_controls(controls(xa), controls(xb), SR, mix_f0=0.5)
    w = definition(xa, xb, mix_f0=0.5)
    got = out["f0"][0, :, 0].numpy()
    print(f"halfway between 200 and 400 Hz: {got[0]:.4f} Hz")
    assert np.abs(got - 200.0 * np.sqrt(2.0)).max() < 2e-5 and np.abs(w["f0"] - 282.8427).max() < 1e-3 and check_f0(got, w) <= 1
    ends = [ddsp.morph_controls(controls(xa), controls(xb), SR, mix_f0=v)["f0"] for v in (0.0, 1.0, -2.0, 7.0)]
    assert (ends[0] == 200).all() and (ends[1] == 400).all() and (ends[2] == 200).all() and (ends[3] == 400).all()    # floats are clamped


def test_voiced_over_unvoiced_fades_at_constant_pitch():
    T = 12
    xa, xb = small_sound(T, 8, 5, f0=220.0), small_sound(T, 8, 5, f0=0.0, seed=6)
    xa["a"][:] = 0.5
    xa["c"][:] = xa["c"][0]
    ramp = torch.linspace(0.0, 1.0, T)
    out = ddsp.morph_controls(controls(xa), controls(xb), SR, mix=ramp)
    a = out["a"][0, :, 0].numpy()
    A = tref.source_amplitudes(xa["f0"], xa["a"], xa["c"], SR)[0].sum()
    err = np.abs(a - (1.0 - ramp.float().double().numpy()) * A).max()
    print(f"voiced over unvoiced, mix 0 -> 1: max |a' - (1 - mix) a| = {err:.3e}")
    assert (out["f0"] == 220.0).all() and err <= 1e-12 and a[-1] == 0 and (out["c"][0, -1] == 1.0 / 8).all()
    silent = ddsp.morph_controls(controls(xb), controls(xb), SR, mix=ramp)                        # neither is present
    assert not silent["f0"].any() and not silent["a"].any() and (silent["c"] == 1.0 / 8).all()
    w = definition(xb, xb, mix=ramp.numpy())
    assert np.abs(silent["H"][0].numpy() - w["N"]).max() <= 1e-12 and w["N"].any()                  # its bands are morphed all the same


def test_each_weight_moves_its_own_part():
    xa, xb = small_sound(10, 30, 9, f0=230.0, seed=7), small_sound(13, 24, 9, f0=410.0, seed=8)
    call = lambda **kw: ddsp.morph_controls(controls(xa), controls(xb), SR, mix=0.4, **kw)         # noqa: E731
    for coordinates in ref.COORDINATES:
        base = call(coordinates=coordinates)
        noise = call(coordinates=coordinates, mix_noise=0.9)
        assert all(torch.equal(noise[k], base[k]) for k in ("f0", "a", "c")) and not torch.equal(noise["H"], base["H"])
        harm = call(coordinates=coordinates, mix_harmonics=0.9)
        assert torch.equal(harm["f0"], base["f0"]) and torch.equal(harm["H"], base["H"]) and not torch.equal(harm["c"], base["c"])
    base, pitch = call(coordinates="harmonic"), call(coordinates="harmonic", mix_f0=0.9)
    assert torch.equal(pitch["H"], base["H"]) and not torch.equal(pitch["f0"], base["f0"])
    k = torch.arange(1, 31)
    audible = (k * pitch["f0"] <= SR // 2) & (k * base["f0"] <= SR // 2)                            # [1, T', H']: not masked in either
    moved = ((pitch["a"] * pitch["c"] - base["a"] * base["c"]).abs() * audible).max()
    assert float(moved) <= 1e-15 and not audible.all() and (pitch["c"][~(k * pitch["f0"] <= SR // 2)] == 0).all()
    hz = call(coordinates="hz", mix_f0=0.9)                      # in Hz coordinates the pitch weight moves the envelope's read-out too
    assert not torch.equal(hz["c"], call(coordinates="hz")["c"])


def test_time_maps_and_frames():
    xa, xb = small_sound(10, 12, 5, f0=230.0, seed=7), small_sound(13, 12, 5, f0=410.0, seed=8)
    for frames, T_out in ((None, 10), (13, 13), (4, 4), (31, 31)):
        out = ddsp.morph_controls(controls(xa), controls(xb), SR, frames=frames)
        w = definition(xa, xb, T_out=T_out)
        assert out["c"].shape == (1, T_out, 12) and out["H"].shape == (1, T_out, 5)
        assert np.abs(amplitudes(out) - ref.morph(dict(xa, pos=ref.linear_positions(10, T_out)), dict(xb, pos=ref.linear_positions(13, T_out)),
                                                  w["wf"], w["wh"], w["wn"], SR, 12, "hz", f0=out["f0"][0, :, 0].numpy())["A"]).max() <= 1e-12
    back = torch.arange(12, -1, -1.0)                            # B reversed: T' = 13, A keeps its linear map onto 13 frames
    out = ddsp.morph_controls(controls(xa), controls(xb), SR, mix=1.0, positions_b=back)
    assert out["a"].shape == (1, 13, 1)
    assert torch.equal(out["H"], ddsp.transform_controls(controls(xb), SR, positions=back)["H"])
    assert ddsp.morph_controls(controls(xa), controls(xb), SR, positions_a=torch.zeros(1, 6), frames=6)["a"].shape == (1, 6, 1)


def test_hostile_per_frame_values_on_the_cpu_path():
    """NaN, infinite and huge weights, positions and pitches follow the silent-frame, clamp and presence rules."""
    T_a, T_b, H, F = 6, 5, 8, 5
    xa, xb = small_sound(T_a, H, F, f0=100.0), small_sound(T_b, H + 3, F, f0=150.0, seed=9)
    xa["f0"][1], xa["f0"][4], xb["f0"][2], xb["f0"][3] = np.nan, np.inf, -np.inf, 1e30
    bad = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, -3.0, 0.0, 2.5], dtype=np.float32)
    n = len(bad)
    cols = np.full((5, 5 * n), 0.5, dtype=np.float32)
    cols[3], cols[4] = 2.5, 0.5
    for i in range(5):
        cols[i, i * n:(i + 1) * n] = bad                         # w_f, w_h, w_n, pos_a, pos_b in turn
    xa["pos"], xb["pos"] = cols[3], cols[4]
    t = torch.from_numpy
    out = ddsp.morph_controls(controls(xa), controls(xb), SR, mix_f0=t(cols[0]), mix_harmonics=t(cols[1]), mix_noise=t(cols[2]),
                              positions_a=t(cols[3]), positions_b=t(cols[4]), n_harmonics=H)
    assert all(torch.isfinite(v).all() for v in out.values())
    f0 = out["f0"][0, :, 0].numpy()
    w = ref.morph(xa, xb, cols[0], cols[1], cols[2], SR, H, "hz", f0=f0)
    assert np.array_equal(w["ma"]["i0"][3 * n:4 * n], [0, T_a - 1, 0, T_a - 1, 0, 0, 0, 2])        # the clamp; a NaN counts as 0
    silent = ~w["sane"]
    assert silent.sum() == 9 and np.array_equal(np.flatnonzero(silent), [0, 1, 2, n, n + 1, n + 2, 2 * n, 2 * n + 1, 2 * n + 2])
    assert not f0[silent].any() and not out["a"][0, silent].any() and (out["c"][0, silent] == 1.0 / H).all() and not out["H"][0, silent].any()
    assert check_f0(f0, w) <= 1 and np.abs(out["c"][0].numpy() - w["c"]).max() <= 1e-12 and np.abs(out["H"][0].numpy() - w["N"]).max() <= 1e-12
    assert np.abs(out["a"][0, :, 0].numpy() - w["a"]).max() <= 1e-12 and (w["a"][~silent] > 0).sum() >= 20


def test_argument_checks():
    xa, xb = small_sound(12, 20, 9), small_sound(10, 16, 9, seed=4)
    A, Bc = controls(xa), controls(xb)
    call = lambda a=A, b=Bc, **kw: ddsp.morph_controls(a, b, SR, **kw)                             # noqa: E731
    two = {k: torch.cat([v, v]) for k, v in Bc.items()}
    for a, b in ((A, two), (A, dict(Bc, H=Bc["H"][..., :5])), (A, {k: v.to("meta") for k, v in Bc.items()}),
                 (A, {k: v for k, v in Bc.items() if k != "H"}), ({k: v for k, v in A.items() if k != "H"}, Bc),
                 (A, {k: v.float() for k, v in Bc.items()}), (A, {k: v for k, v in Bc.items() if k != "a"}),
                 (dict(A, f0=A["f0"][..., 0]), Bc), (A, dict(Bc, c=Bc["c"][:, :-1]))):
        with pytest.raises(ValueError):                          # batch, bands, device, H in one dict only, dtype, keys, shapes
            call(a, b)
    for kw in (dict(frames=7, positions_a=torch.zeros(6)), dict(positions_a=torch.zeros(6), positions_b=torch.zeros(7)),
               dict(frames=0), dict(mix=float("nan")), dict(mix_f0=float("inf")), dict(mix_noise=-float("inf")), dict(coordinates="mel"),
               dict(coordinates=0), dict(n_harmonics=0), dict(mix=torch.zeros(5)), dict(mix_harmonics=torch.zeros(2, 12)),
               dict(positions_b=torch.zeros(2, 12)), dict(positions_a=[0.0] * 12), dict(mix=torch.zeros(12, device="meta"))):
        with pytest.raises(ValueError):
            call(**kw)
    for key in ("f0", "a", "c", "H"):                            # no backward: refused as the analysis refuses it
        with pytest.raises((ValueError, RuntimeError)):
            call(A, dict(Bc, **{key: Bc[key].clone().requires_grad_()}))
    with pytest.raises((ValueError, RuntimeError)):
        call(mix=torch.zeros(12, requires_grad=True))
    empty = call({k: v[:0] for k, v in A.items()}, {k: v[:0] for k, v in Bc.items()}, frames=18, n_harmonics=7)
    assert empty["f0"].shape == empty["a"].shape == (0, 18, 1) and empty["c"].shape == (0, 18, 7) and empty["H"].shape == (0, 18, 9)
    bare = call({k: v for k, v in A.items() if k != "H"}, {k: v for k, v in Bc.items() if k != "H"})
    assert sorted(bare) == ["a", "c", "f0"] and bare["c"].shape == (1, 12, 20)


def test_symbol_is_bound_and_the_abi_is_still_5():
    text = open(os.path.join(ROOT, "include", "ddsp_hip.h")).read()
    assert re.search(r"\bint\s+ddsp_morph_controls\s*\(", text)
    assert text.index("ddsp_transform_controls(") < text.index("ddsp_morph_controls(") < text.index("int ddsp_loudness_supported(")
    order = list(ddsp._lib.EXPORTS)
    assert order[order.index("ddsp_transform_controls") + 1] == "ddsp_morph_controls"             # the table keeps the header's order
    L = ddsp._lib.lib()
    assert L.ddsp_hip_abi_version() == 5 == ddsp._lib.ABI_VERSION
    assert L.ddsp_morph_controls.restype is ctypes.c_int
    assert list(L.ddsp_morph_controls.argtypes) == ([ctypes.c_void_p] * 17 + [ctypes.c_long] * 4 + [ctypes.c_int] * 6 + [ctypes.c_void_p])
    assert re.search(r"#define\s+DDSP_MORPH_HZ\s+0\b", text) and re.search(r"#define\s+DDSP_MORPH_HARMONIC\s+1\b", text)
    assert ddsp.analysis.MORPH_COORDINATES == dict(hz=0, harmonic=1)


def test_entry_point_checks_return_before_any_launch():
    """Every call here is refused (or is the empty batch) by the host checks: the pointers are never dereferenced."""
    L = ddsp._lib.lib()
    p, N = 4096, None                                            # a non-null address that is never read
    def call(ptrs, B=2, T_a=16, T_b=12, T_out=24, H_a=20, H_b=30, H_out=20, F=65, sr=16000, coordinates=0):
        return L.ddsp_morph_controls(*ptrs, B, T_a, T_b, T_out, H_a, H_b, H_out, F, sr, coordinates, N)
    good = (p,) * 17
    noise = (3, 8, 16)
    bare = tuple(N if k in noise else p for k in range(17))      # no noise in, none out
    assert call((N,) * 17, B=0) == 0
    for i in set(range(17)) - set(noise):
        assert call(tuple(N if k == i else v for k, v in enumerate(good))) == EINVAL, i
        assert call(tuple(N if k == i else v for k, v in enumerate(bare))) == EINVAL, i
    for gone in ((3,), (8,), (16,), (3, 8), (3, 16), (8, 16)):    # the three noise pointers: all or none
        assert call(tuple(N if k in gone else v for k, v in enumerate(good))) == EINVAL, gone
    for kw in (dict(B=-1), dict(T_a=0), dict(T_b=0), dict(T_out=0), dict(H_a=0), dict(H_b=0), dict(H_out=0), dict(F=0), dict(sr=0),
               dict(T_b=-4), dict(H_out=-1), dict(coordinates=2), dict(coordinates=-1)):
        assert call(good, **kw) == EINVAL and call(bare, **kw) == EINVAL, kw
    for kw in (dict(H_a=257), dict(H_b=257), dict(H_out=257), dict(F=258), dict(B=1 << 30, T_a=1 << 30), dict(B=1 << 30, T_b=1 << 30),
               dict(B=1 << 30, T_out=1 << 30), dict(B=1 << 40, T_b=1 << 40), dict(B=(1 << 24) + 1, T_a=1 << 23)):
        assert call(good, **kw) == ERANGE and call(bare, **kw) == ERANGE, kw
    # the order: pointers, signs and the coordinates before ranges
    assert call((N,) * 17, H_a=257) == EINVAL and call(good, H_b=257, T_a=0) == EINVAL and call(good, F=258, coordinates=5) == EINVAL


def test_device_bound():
    """TOL_M from the kernel's arithmetic on the device tests' own inputs (see the module's docstring), the generators' distance
    from Nyquist, and the branches the inputs reach."""
    fig_a = fig_n = 0.0
    reached, margin = {}, np.inf
    assert ref.GRID_SHAPE[3] == ddsp.analysis.MORPH_KERNEL_MAX_BLOCKS * ddsp.analysis.MORPH_KERNEL_WAVES + 5
    for shape, coordinates in CASES + [(ref.GRID_SHAPE, "hz")]:
        B, T_a, T_b, T_out, H_a, H_b, H_out, F = shape
        x = ref.rows(shape)
        for b in range(B):
            args = (*ref.row_of(x, b), SR, H_out, coordinates)
            w, g = ref.morph(*args), ref.morph_fp32(*args)
            assert np.array_equal(g["f0"].view(np.uint32), w["f0"].view(np.uint32))
            margin = min(margin, ref.nyquist_margin(w["f0"], SR, H_out))
            A = g["a"].astype(np.float64)[:, None] * g["c"].astype(np.float64) * (g["a"] != 0)[:, None]
            assert np.array_equal(A == 0, w["A"] == 0) and np.array_equal(g["N"] == 0, w["N"] == 0)
            loud, hiss = w["scale"] > 0, w["nscale"] > 0
            ea = (np.abs(A - w["A"])[loud] / w["scale"][loud, None]).max() if loud.any() else 0.0
            en = (np.abs(g["N"] - w["N"])[hiss] / w["nscale"][hiss, None]).max() if hiss.any() else 0.0
            print(f"{shape} {coordinates} row {b}: fp32 arithmetic, A' {ea:.3e}, N' {en:.3e} of the largest source value")
            fig_a, fig_n = max(fig_a, ea), max(fig_n, en)
            for key, value in ref.branches(w, ref.row_of(x, b)).items():
                reached[key] = reached.get(key, 0) + value
    print(f"derived bound: 2 x max({fig_a:.3e}, {fig_n:.3e}) = {2 * max(fig_a, fig_n):.3e}; TOL_M = {ref.TOL_M:g}; "
          f"fl32(k' f0') at least {margin:.1f} ulp from Nyquist; branches {reached}")
    assert margin >= 4
    assert all(reached.values()), reached
    assert 2 * max(fig_a, fig_n) <= ref.TOL_M <= 1e-5
    assert ref.TOL_M <= 1.5 * 2 * max(fig_a, fig_n)                                              # twice the figure, rounded up: no more
