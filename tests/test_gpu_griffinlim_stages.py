"""Griffin-Lim's three kernels (csrc/ddsp_griffinlim.hip: synthesis, overlap-add, analysis) one at a time, through the test hook
ddsp_griffinlim_stage, against the fp64 reference and the derived bounds of tests/griffinlim_reference.py: each stage alone at
every n_fft and at the shapes where the indexing can go wrong, spec_at under designed conditioning, teacher-forced single steps
along the G27 trajectories (the per-step answer to what the free-running comparison of tests/test_gpu_griffinlim.py cannot
tell), and the grid-stride loops beyond their caps.  Every test prints the figures it asserts on (`pytest -s`)."""
import functools

import numpy as np
import pytest
import torch

import ddsp_pytorch_amd as ddsp

import griffinlim_reference as G

pytestmark = pytest.mark.gpu

U = G.U
SHAPE_IDS = [s[0] for s in G.GPU_SHAPES]


def show(lines):
    for line in lines:
        print(line)


# ---- a. each stage alone ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SHAPE_IDS)
def test_synthesis_alone(name):
    """Every form of spec_at's input: no R (all-one angles, given angles), R alone, R and Rprev, and c == 0 with both."""
    p = G.shape_setup(G.SHAPE_BY_NAME[name])
    n, hop, B, T, L, w = (p[k] for k in ("n_fft", "hop", "B", "T", "L", "window"))
    c = float(np.float32(0.9 / 1.9))
    S, ang0, R, Rprev = G.random_state(n + T, B, T, n, c)
    lines, ok = [], True
    for tag, state in (("ones", dict()), ("ang0", dict(ang0=ang0)), ("R", dict(R=R, c=c)), ("R,Rprev", dict(R=R, Rprev=Rprev, c=c)),
                       ("R,Rprev,c=0", dict(R=R, Rprev=Rprev, c=0.0))):
        got = G.device_synth(S, w, hop, L, **state)
        ok &= G.check_synth(f"{name} {tag}", got, S, w, lines=lines, **state)[0]
        if tag == "R,Rprev,c=0":                                 # R - 0 * Rprev == R: the same bits as without Rprev
            ok &= np.array_equal(G.bits(got), G.bits(G.device_synth(S, w, hop, L, R=R, c=0.0)))
        if tag == "ang0":                                        # angles are read only without R
            ok &= np.array_equal(G.bits(G.device_synth(S, w, hop, L, ang0=ang0, R=R, c=c)), G.bits(G.device_synth(S, w, hop, L, R=R, c=c)))
    show(lines)
    assert ok


@pytest.mark.parametrize("name", SHAPE_IDS)
def test_analysis_alone(name):
    p = G.shape_setup(G.SHAPE_BY_NAME[name])
    y = G.f32(np.random.default_rng(p["n_fft"] + 1).standard_normal((p["B"], p["L"])))
    got = G.device_analysis(y, p["window"], p["hop"], p["T"])
    ok, lines = G.check_analysis(name, got, y, p["window"], p["hop"])
    show(lines)
    assert ok


@pytest.mark.parametrize("name", SHAPE_IDS)
def test_overlap_alone(name):
    p = G.shape_setup(G.SHAPE_BY_NAME[name])
    fr = G.f32(np.random.default_rng(p["n_fft"] + 2).standard_normal((p["B"], p["T"], p["n_fft"])))
    got = G.device_overlap(fr, p["env"], p["hop"], p["L"])
    ok, lines = G.check_overlap(name, got, fr, p["env"], p["hop"], p["L"])
    show(lines)
    assert ok
    if name == "n64_rect_zero_tail":
        assert p["L"] - G.natural_length(64, 64, p["T"]) == 18 and np.all(G.bits(got[:, -18:]) == 0) and np.all(got[:, :-18] != 0)


def test_the_2048_in_row_path_and_the_reflected_path_give_the_same_bits():
    """hop 512: frame 4 reads samples 1024 .. 3071.  At L = 3072 it lies inside the row (the fast path, with equality); at
    L = 3071 its last sample is the reflection of 3071, which is sample 3069.  With y[3071] = y[3069] both read the same values:
    the same bits, as do the interior frames 1 .. 3 of both (in-row in both)."""
    a, b = G.shape_setup(G.SHAPE_BY_NAME["n2048_h512_L3072"]), G.shape_setup(G.SHAPE_BY_NAME["n2048_h512_L3071"])
    y = G.f32(np.random.default_rng(7).standard_normal((a["B"], 3072)))
    y[:, 3071] = y[:, 3069]
    Ra = G.device_analysis(y, a["window"], 512, a["T"])
    Rb = G.device_analysis(y[:, :3071], b["window"], 512, b["T"])
    assert Ra.shape[1] == 7 and Rb.shape[1] == 6
    assert np.array_equal(G.bits(Ra[:, 1:5]), G.bits(Rb[:, 1:5]))
    assert not np.array_equal(G.bits(Ra[:, 5]), G.bits(Rb[:, 5]))         # (frame 5 reflects other samples in the two)
    for tag, got, yy in (("L3072", Ra, y), ("L3071", Rb, y[:, :3071])):
        ok, lines = G.check_analysis(tag, got, yy, a["window"], 512)
        show(lines)
        assert ok


@pytest.mark.parametrize("n_iter", [0, 2])
def test_zero_tail_through_the_public_entry(n_iter):
    """A rectangular window with hop = n_fft and `length` 18 samples past the natural length: spectral.py pads the envelope it
    hands to the library.  Against the fp64 loop on torch.istft / torch.stft: the tail exactly 0, the rest within CPU_FACTOR
    times the stock fp32 loop's error on the CPU."""
    from ddsp_pytorch_amd import spectral
    p = G.shape_setup(G.SHAPE_BY_NAME["n64_rect_zero_tail"])
    n, hop, B, T, L = p["n_fft"], p["hop"], p["B"], p["T"], p["L"]
    S, ang0, _, _ = G.random_state(18, B, T, n, 0.0)
    spec = torch.from_numpy(np.ascontiguousarray(np.transpose(S, (0, 2, 1)))).float()
    angles = torch.from_numpy(np.ascontiguousarray(np.transpose(ang0, (0, 2, 1)))).to(torch.complex64)
    w = torch.ones(n)
    y = ddsp.griffinlim(spec.cuda(), w.cuda(), n, hop, n, 1.0, n_iter, 0.5, L, False, angles=angles.cuda()).cpu().numpy()
    stock = spectral._stock_loop(spec, torch.view_as_real(angles).contiguous(), w, n, hop, n, n_iter, 0.5, L).numpy()
    c = float(np.float32(0.5 / 1.5))
    env = G.envelope(p["window"], hop, T, L)
    Rs = G.trajectory(S, ang0, p["window"], env, hop, L, c, n_iter)
    state = dict(ang0=ang0) if n_iter == 0 else dict(R=Rs[-1], Rprev=Rs[-2], c=c)
    exact = G.overlap(G.synth(S, p["window"], **state), env, hop, L)
    err, cpu = np.abs(y - exact).max(), np.abs(stock - exact).max()
    print(f"GLS zero tail, n_iter {n_iter}: gpu {err:.3e} cpu {cpu:.3e}")
    assert y.shape == (B, L) and np.all(G.bits(y[:, -18:]) == 0) and np.all(exact[:, -18:] == 0)
    assert err <= G.CPU_FACTOR * cpu


# ---- b. spec_at under designed conditioning ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", G.SIZES)
def test_spec_at_under_designed_conditioning(n):
    """Synthesis with an all-ones window; the spectrum recovered by an fp64 rfft of the device's frames.  Every bin within
    S (2 kappa U + 3 U) plus the transform's floor: CPU_FACTOR times the largest per-bin error, in that frame, of the CPU fp32
    irfft of the (fp32-rounded) exact spectrum, recovered the same way -- measured from the library, never from the device."""
    B, T = 3, 7
    S, R, Rprev, c, ill = G.designed_state(n, B, T, n)
    k = G.kappa(R, Rprev, c)
    assert k[..., ~ill].max() <= 2.0 and (~ill).mean() >= 15.0 / 16.0 and k[..., ill].max() >= (2.0e4 if n >= 512 else 100.0)
    ones = np.ones(n)
    got = G.device_synth(S, ones, n, n * (T - 1), R=R, Rprev=Rprev, c=c).astype(np.float64)
    X = G.spectrum(S, R=R, Rprev=Rprev, c=c)
    X32 = G.f32(X)
    cpu = torch.fft.irfft(torch.from_numpy(X32).to(torch.complex64), n=n, dim=-1).numpy().astype(np.float64)
    floor = G.CPU_FACTOR * np.abs(np.fft.rfft(cpu, axis=-1) - X32).max(axis=-1, keepdims=True)
    err = np.abs(np.fft.rfft(got, axis=-1) - X)
    bound = G.spec_bound(S, R, Rprev, c)
    ratio = err / (bound + floor)                                # every bin of every frame: none is excluded
    scale = np.linalg.norm(X, axis=-1, keepdims=True) / np.sqrt(n)
    print(f"GLS spec_at n{n}: kappa max {k.max():.3g}; worst error / (bound + floor): all {ratio.max():.3f}, ill-conditioned "
          f"{ratio[..., ill].max():.3f} (error / bound alone {(err / bound)[..., ill].max():.3f}), well-conditioned {ratio[..., ~ill].max():.3f}; "
          f"floor {float((floor / G.CPU_FACTOR / scale).min()) / U:.1f} .. {float((floor / G.CPU_FACTOR / scale).max()) / U:.1f} U |X|_2 / sqrt(n)")
    assert ratio.shape == (B, T, n // 2 + 1) and np.isfinite(ratio).all()
    assert ratio.max() <= 1.0


# ---- c. teacher-forced steps along the G27 trajectories ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def g27_states(golden, case):
    """The fixture's setup and its teacher-forced states, the fp64 trajectory computed once."""
    p = G.g27_setup(golden("g27_" + case))
    return p, G.teacher_forced_states(p)


def within(gpu_worst, cpu_worst, err, bound):
    """At most CPU_FACTOR times the CPU stock step's worst figure, or everywhere within the conditioned bound."""
    return bool(gpu_worst <= G.CPU_FACTOR * cpu_worst or np.all(err <= bound))


@pytest.mark.parametrize("case", G.G27)
def test_teacher_forced_steps_along_g27(golden, case):
    """k = 1 .. 16: from (S, R_(k-1), R_(k-2)) of the fp64 trajectory rounded to fp32, ONE device step through the three stages
    (each fed the device's own output of the one before) against the fp64 step from the same inputs: frames and R_k per frame
    and y per row, in the 2-norm -- each within CPU_FACTOR times the CPU stock fp32 step's error from the same inputs, or within
    the conditioned bound of spec_at carried through the step (G.step_bounds without the transforms' ceilings), whichever is
    larger."""
    p, states = g27_states(golden, case)
    S, w, env, hop, L, c, T = (p[k] for k in ("S", "window", "env", "hop", "L", "c", "T"))
    bad = []
    for k, R, Rprev in states:
        state = dict(R=R, Rprev=Rprev, c=c)
        fr, y, Rn = G.step(S, w, env, hop, L, **state)
        sf, sy, sR = G.stock_step(S, w, hop, L, **state)
        fb, yb, rb = G.step_bounds(S, w, env, hop, L, ceilings=False, **state)
        d_fr = G.device_synth(S, w, hop, L, **state)
        d_y = G.device_overlap(d_fr, env, hop, L)
        d_R = G.device_analysis(d_y, w, hop, T)
        ef, cf = G.frame_err(d_fr.astype(np.float64), fr), G.frame_err(sf, fr)
        ey, cy = G.frame_err(d_y.astype(np.float64), y), G.frame_err(sy, y)
        er, cr = G.frame_err(d_R.astype(np.complex128), Rn), G.frame_err(sR, Rn)
        gf, hf, gy, hy, gr, hr = (G.rel(e, ref).max() for e, ref in ((ef, fr), (cf, fr), (ey, y), (cy, y), (er, Rn), (cr, Rn)))
        kap = G.kappa(R, Rprev, c)
        ok = within(gf, hf, ef, fb) and within(gy, hy, ey, yb) and within(gr, hr, er, rb)
        print(f"GLS step {case} k={k:2d}: kappa max {kap.max():9.3g} | frames gpu {gf / U:5.2f}U cpu {hf / U:5.2f}U conditioned {G.rel(fb, fr).max() / U:7.1f}U"
              f" | y gpu {gy / U:5.2f}U cpu {hy / U:5.2f}U conditioned {G.rel(yb, y).max() / U:7.1f}U, max |dy| gpu {np.abs(d_y - y).max():.2e} cpu "
              f"{np.abs(sy - y).max():.2e} | R_k gpu {gr / U:5.2f}U cpu {hr / U:5.2f}U conditioned {G.rel(rb, Rn).max() / U:8.1f}U"
              f"{'' if ok else '   <-- OUT OF BOUND'}")
        if not ok:
            bad.append(k)
    assert not bad, (case, bad)


# ---- d. beyond the grids ----------------------------------------------------------------------------------------------------
def even_blocks(cap_frames, total):
    """Even-aligned runs of flat frame indices: the first frames, either side of the cap, and the last ones."""
    return [(0, 4), (cap_frames - 4, cap_frames + 4), ((total - 5) // 2 * 2, total)]


def flat(a, lo, hi):
    """Frames lo .. hi of the flat frame order of a [B, T, ...] array, as a [1, hi - lo, ...] batch."""
    return a.reshape((-1,) + a.shape[2:])[lo:hi][None]


@pytest.mark.parametrize("n,B,T,hop", [(64, 8195, 33, 16), (2048, 497, 33, 512)], ids=["n64", "n2048"])
def test_synthesis_and_analysis_with_more_units_than_the_grid(n, B, T, hop):
    """More than 16384 units (16 frames a unit at 64 points, one at 2048): the first blocks walk a second unit.  The frames either
    side of the cap and the last ones against fp64 under the criteria of the stages alone; everything finite; the last row
    launched alone (other blocks, other turns of the stride) has the same bits as inside the batch."""
    cap = G.MAX_UNITS * G.frames_per_unit(n)
    total = B * T
    assert total > cap and (B - 1) * T % 2 == 0                   # (the last row starts a pair, alone and in the batch)
    L = hop * (T - 1)
    w = G.f32(G.hann(n))
    rng = np.random.default_rng(n)
    F = n // 2 + 1
    S = rng.random((B, T, F), dtype=np.float32) + np.float32(0.01)
    R = (rng.standard_normal((B, T, F), dtype=np.float32) + 1j * rng.standard_normal((B, T, F), dtype=np.float32)).astype(np.complex64)
    Rprev = np.roll(R, 1, axis=0) * np.complex64(1j) if n == 64 else None
    c = float(np.float32(0.3))
    dS, dR, dP = (G.to_device(S), G.to_device(R, True), G.to_device(Rprev, True))
    fr = G.device_synth(dS, w, hop, L, R=dR, Rprev=dP, c=c)
    assert fr.shape == (B, T, n) and np.isfinite(fr).all()
    lines, ok = [], True
    for lo, hi in even_blocks(cap, total):
        state = dict(R=flat(R, lo, hi).astype(np.complex128), c=c)
        if Rprev is not None:
            state["Rprev"] = flat(Rprev, lo, hi).astype(np.complex128)
        ok &= G.check_synth(f"n{n} frames {lo}..{hi - 1}", flat(fr, lo, hi), flat(S, lo, hi).astype(np.float64), w, lines=lines, **state)[0]
    alone = G.device_synth(S[-1:], w, hop, L, R=R[-1:], Rprev=None if Rprev is None else Rprev[-1:], c=c)
    ok &= np.array_equal(G.bits(alone[0]), G.bits(fr[-1]))
    del dS, dR, dP, fr, R, Rprev, S

    y = rng.standard_normal((B, L), dtype=np.float32)
    Rg = G.device_analysis(y, w, hop, T)
    assert Rg.shape == (B, T, F) and np.isfinite(Rg.view(np.float32)).all()
    for lo, hi in even_blocks(cap, total):
        rows = sorted({lo // T, (hi - 1) // T})
        ref = G.analysis(y[rows].astype(np.float64), w, hop, T)
        cpu = G.stock_analysis(y[rows], w, hop)
        sel = [(rows.index(f // T), f % T) for f in range(lo, hi)]
        pick = lambda a: np.stack([a[r, t] for r, t in sel])[None]                               # noqa: E731
        got = flat(Rg, lo, hi).astype(np.complex128)
        ok &= G.sharp(f"n{n} frames {lo}..{hi - 1} analysis", G.frame_err(got, pick(ref)), pick(ref), G.frame_err(pick(cpu), pick(ref)),
                      G.analysis_ceiling(pick(ref), n), lines)
    ok &= np.array_equal(G.bits(G.device_analysis(y[-1:], w, hop, T)[0]), G.bits(Rg[-1]))
    show(lines)
    assert ok


def test_overlap_with_more_samples_than_the_grid():
    """B L > 65536 * 256 samples at n_fft 64: the first threads walk a second sample.  The whole output bit for bit against the
    fp32 restatement; the rows either side of the cap and the last one within the summation bound of the fp64 sum; the last
    row launched alone has the same bits."""
    n, hop, B, L = 64, 16, 4097, 4100
    T = 1 + L // hop
    assert B * L > G.MAX_OVERLAP_THREADS
    rng = np.random.default_rng(64)
    fr = rng.standard_normal((B, T, n), dtype=np.float32)
    env = (0.5 + 1.5 * rng.random(L)).astype(np.float32)
    got = G.device_overlap(fr, env, hop, L)
    want = G.overlap_fp32(fr, env, hop, L)
    differing = int((G.bits(got) != G.bits(want)).sum())
    rows = sorted({0, G.MAX_OVERLAP_THREADS // L - 1, G.MAX_OVERLAP_THREADS // L, G.MAX_OVERLAP_THREADS // L + 1, B - 1})
    f64 = fr[rows].astype(np.float64)
    ratio = np.abs(got[rows] - G.overlap(f64, env, hop, L)) / G.overlap_bound(f64, env, hop, L)
    print(f"GLS overlap beyond the grid: {differing} of {got.size} samples differ from the fp32 restatement; rows {rows}: worst error / "
          f"summation bound {ratio.max():.3f}")
    assert np.isfinite(got).all() and differing == 0 and ratio.max() <= 1.0
    assert np.array_equal(G.bits(G.device_overlap(fr[-1:], env, hop, L)[0]), G.bits(got[-1]))
