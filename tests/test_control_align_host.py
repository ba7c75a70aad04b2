"""The time alignment without a GPU: the definition of tests/control_align_reference.py against a brute
force, the package's torch path against it (exactly in fp32, exactly in fp64), the properties the alignment is for, the two derived
tolerances, and the argument checks."""
import numpy as np
import pytest
import torch

import ddsp_pytorch_amd as ddsp
import control_align_reference as ref
from ddsp_pytorch_amd import analysis
from encoder_common import AEConf

SR = ref.SAMPLE_RATE


def cpu(x, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype)


def controls(x, dtype=torch.float32, noise=True):
    out = dict(f0=cpu(x["f0"], dtype)[None, :, None], a=cpu(x["a"], dtype)[None, :, None], c=cpu(x["c"], dtype)[None])
    if noise and x.get("N") is not None:
        out["H"] = cpu(x["N"], dtype)[None]
    return out


def row_of(ctrl):
    """A control dict of one row -> the arrays the reference takes."""
    out = {k: ctrl[k][0, :, 0].numpy() for k in ("f0", "a")}
    out["c"], out["N"] = ctrl["c"][0].numpy(), ctrl["H"][0].numpy() if "H" in ctrl else None
    return out


def test_the_definition_is_the_best_of_all_monotone_paths():
    rng = np.random.default_rng(3)
    worst, count = 0.0, 0
    for T_a in range(1, 5):
        for T_b in range(1, 5):
            for radius, penalty in ((None, 0.0), (None, 0.3), (1, 0.0), (1, 0.3), (2, 0.05)):
                xa, xb = rng.normal(size=(T_a, 2)), rng.normal(size=(T_b, 2))
                path, cost = ref.dtw(xa, xb, radius, penalty)
                best = ref.brute_force(xa, xb, radius, penalty)
                assert np.isfinite(best)
                worst = max(worst, abs(cost - best), abs(ref.path_cost(path, xa, xb, radius, penalty) - best))
                count += 1
    print(f"the recurrence against every monotone path on {count} tiny inputs: |cost - best| <= {worst:.3e}")
    assert worst <= 1e-13


@pytest.mark.parametrize("case", ref.GPU_CASES, ids=str)
def test_torch_path_is_the_emulation_in_fp32_and_the_definition_in_fp64(case):
    B, T_a, T_b, D, radius, penalty = case
    xa, xb = ref.sequences(B, T_a, T_b, D)
    for dtype, np_dtype in ((torch.float32, np.float32), (torch.float64, np.float64)):
        pos_a, pos_b, path, length, cost = ddsp.dtw_align(cpu(xa, dtype), cpu(xb, dtype), radius=radius, penalty=penalty, timing=0.5,
                                                          return_path=True)
        assert path.dtype == torch.int32 and length.dtype == torch.int32 and cost.dtype == dtype and pos_a.dtype == torch.float32
        for b in range(B):
            want, want_cost = ref.dtw(xa[b], xb[b], radius, penalty, np_dtype)
            n = int(length[b])
            assert n == len(want) and np.array_equal(path[b, :n].numpy(), want) and bool((path[b, n:] == -1).all())
            assert max(T_a, T_b) <= n <= T_a + T_b - 1
            assert np_dtype(want_cost) == cost[b].numpy()
            wa, wb = ref.timeline(want, T_a, T_b, 0.5)
            assert np.array_equal(wa.astype(np.float32), pos_a[b].numpy()) and np.array_equal(wb.astype(np.float32), pos_b[b].numpy())


@pytest.mark.parametrize("T_a,D", ref.WARP_SHAPES)
def test_warped_copies_are_found_exactly(T_a, D):
    xa, xb, w = ref.warped_copy(T_a, D)
    T_b = len(w)
    d = ref.local_costs(xa, xb, np.float32)
    assert np.array_equal(np.argwhere(d == 0), np.stack([w, np.arange(T_b)], 1)[np.lexsort((np.arange(T_b), w))])
    for tau in (0.0, 1.0):
        pos_a, pos_b, path, length, cost = ddsp.dtw_align(cpu(xa)[None], cpu(xb)[None], timing=tau, return_path=True)
        assert int(length[0]) == T_b and np.array_equal(path[0, :T_b].numpy(), np.stack([w, np.arange(T_b)], 1)) and float(cost[0]) == 0.0
        if tau == 1.0:
            assert np.array_equal(pos_b[0].numpy(), np.arange(T_b, dtype=np.float32)) and np.array_equal(pos_a[0].numpy(), w.astype(np.float32))
        else:
            assert np.array_equal(pos_a[0].numpy(), np.arange(T_a, dtype=np.float32)) and bool((pos_b[0].diff() >= 0).all())
            assert float(pos_b[0, 0]) >= 0 and float(pos_b[0, -1]) <= T_b - 1


def test_timeline():
    xa, xb = ref.sequences(1, 37, 50, 5)
    path, _ = ref.dtw(xa[0], xb[0], None, 0.01)
    for frames in (None, 1, 2, 29, 200):
        pa, pb = ref.timeline(path, 37, 50, 0.5, frames)
        T_out = ref.default_frames(37, 50, 0.5) if frames is None else frames
        assert len(pa) == T_out == len(pb) and (np.diff(pa) >= 0).all() and (np.diff(pb) >= 0).all()
        assert (pa[0], pb[0]) == (0.0, 0.0) and (T_out == 1 or (pa[-1], pb[-1]) == (36.0, 49.0))
        ramp = np.arange(T_out) * (0.5 * 36 + 0.5 * 49) / max(1, T_out - 1)
        off = np.abs(0.5 * pa + 0.5 * pb - ramp).max()
        print(f"T' = {T_out}: |(1 - tau) pos_a + tau pos_b - ramp| <= {off:.3e}")
        assert off <= 1e-12
        got = ddsp.dtw_align(cpu(xa), cpu(xb), penalty=0.01, timing=0.5, frames=frames)
        assert got[0].shape == (1, T_out)
    assert ref.default_frames(37, 50, 0.5) == 44 and ddsp.dtw_align(cpu(xa), cpu(xb), timing=7.0)[0].shape == (1, 50)   # tau is clamped


@pytest.mark.parametrize("T_a,T_b", ref.BAND_SHAPES)
def test_band(T_a, T_b):
    inside = ref.allowed(T_a, T_b, 1)
    p, q = T_a - 1, T_b - 1
    for i in range(T_a):
        for j in range(T_b):
            assert inside[i, j] == (abs(i * q - j * p) <= max(p, q))
    xa, xb = ref.sequences(1, T_a, T_b, 3)
    for penalty in (0.0, 0.01):
        path, cost = ref.dtw_fp32(xa[0], xb[0], 1, penalty)
        assert np.isfinite(cost) and inside[path[:, 0], path[:, 1]].all()                      # the end is reachable
        _, _, got, length, _ = ddsp.dtw_align(cpu(xa), cpu(xb), radius=1, penalty=penalty, return_path=True)
        assert np.array_equal(got[0, :int(length[0])].numpy(), path)


def test_a_large_penalty_forces_the_diagonal():
    xa, xb = ref.sequences(2, 23, 23, 4)
    pos_a, pos_b, path, length, _ = ddsp.dtw_align(cpu(xa), cpu(xb), penalty=1e6, return_path=True)
    assert bool((length == 23).all()) and bool((path[:, :23, 0] == path[:, :23, 1]).all())
    assert torch.equal(pos_a, pos_b) and torch.equal(pos_a[0], torch.arange(23.0))


def test_fp32_paths_cost_what_the_fp64_optimum_costs():
    """TOL_P: the excess of the emulation's path over the fp64 optimum, both scored in fp64, relative to the optimum + 1, on the
    device tests' inputs.  Measured: 0 -- the paths differ on one input ((1, 129, 200, 42), no band, penalty 0.01), through a tie in
    fp64.  Twice that is 0, so the bound is the scoring's own noise: a sum of at most 328 fp64 terms, 328 x 1.2e-16 < 1e-12 = TOL_P."""
    worst, differ = 0.0, 0
    for B, T_a, T_b, D, radius, penalty in ref.GPU_CASES:
        xa, xb = ref.sequences(B, T_a, T_b, D)
        for b in range(B):
            p32, _ = ref.dtw_fp32(xa[b], xb[b], radius, penalty)
            p64, _ = ref.dtw(xa[b], xb[b], radius, penalty)
            best = ref.path_cost(p64, xa[b], xb[b], radius, penalty)
            worst = max(worst, (ref.path_cost(p32, xa[b], xb[b], radius, penalty) - best) / (best + 1.0))
            differ += not (len(p32) == len(p64) and np.array_equal(p32, p64))
    print(f"fp32 paths scored in fp64: excess {worst:.3e} of the optimum + 1 (TOL_P {ref.TOL_P:g}); {differ} paths differ from fp64's")
    assert worst <= ref.TOL_P and ref.TOL_P <= max(1.5 * 2 * worst, 1e-12)


def feature_inputs():
    """-> [(name, control row)]: the phrase (an unvoiced run), its transposed second take, random controls, a silent row, F = 2."""
    A, w = ref.phrase()
    second = row_of(ddsp.transform_controls(controls(A), SR, positions=cpu(w), transpose=5.0, formant=0.0))
    x = ref.tref.rows((3, 9, 9, 23, 23, 2))
    random = [dict(f0=x["f0"][b], a=x["a"][b], c=x["c"][b], N=x["N"][b]) for b in range(3)]           # F = 2: empty noise groups
    silent = dict(A, a=np.zeros_like(A["a"]), N=np.zeros_like(A["N"]))
    return [("phrase", A), ("second take", second), ("silent", silent)] + [(f"random {b}", r) for b, r in enumerate(random)]


def test_features_match_their_definition():
    """TOL_F: the fp32 emulation of the features against fp64 on these inputs, doubled and rounded up; the package's CPU path is
    held to it, with and without the noise bands, and is the definition itself in fp64."""
    emulated = measured = 0.0
    for name, x in feature_inputs():
        for noise in (True, False):
            N = x["N"] if noise else None
            want = ref.features(x["f0"], x["a"], x["c"], N, SR)
            emulated = max(emulated, np.abs(ref.features(x["f0"], x["a"], x["c"], N, SR, dtype=np.float32) - want).max())
            got = ddsp.control_features(controls(x, noise=noise), SR)
            D = 32 + 2 + (8 if noise else 0)
            assert got.shape == (1, len(x["f0"]), D) == (1,) + want.shape and got.dtype == torch.float32
            assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0
            measured = max(measured, np.abs(got[0].numpy() - want).max())
            exact = np.abs(ddsp.control_features(controls(x, torch.float64, noise), SR)[0].numpy() - want).max()
            assert exact <= 1e-14, (name, exact)
            if name == "silent":
                assert not want[:, :-1].any()                                                      # every part at its floor
    print(f"features: emulation {emulated:.3e}, package {measured:.3e} from fp64 (TOL_F {ref.TOL_F:g})")
    assert emulated <= ref.TOL_F / 2 and ref.TOL_F <= 1.5 * 2 * emulated and measured <= ref.TOL_F
    other = ddsp.control_features(controls(feature_inputs()[0][1]), SR, n_bands=20, noise_groups=3, range_log2=6.0)
    assert other.shape == (1, 48, 25)


def test_a_phrase_aligns_with_its_slower_transposed_take():
    """The cap, not a measurement: every path point (i, j) has i and w(j) in one segment, and |i - w(j)| <= 1."""
    A, w = ref.phrase()
    ctrl_a = controls(A)
    ctrl_b = ddsp.transform_controls(ctrl_a, SR, positions=cpu(w), transpose=5.0, formant=0.0)
    assert ctrl_b["f0"].shape == (1, 71, 1) and abs(float(ctrl_b["f0"][0, 0, 0]) / 200.0 - 2.0 ** (5 / 12)) < 1e-6
    for penalty in (0.0, 0.01):
        pos_a, pos_b, path, length, cost = ddsp.align_controls(ctrl_a, ctrl_b, SR, penalty=penalty, return_path=True)
        wrong, off = ref.phrase_deviation(path[0, :int(length[0])].numpy().astype(np.int64), w)
        print(f"penalty {penalty}: {int(length[0])} path points, {wrong} across segments, |i - w(j)| <= {off}, cost {float(cost[0]):.4f}")
        assert wrong == 0 and off <= 1
        assert torch.equal(pos_a[0], torch.arange(48.0))
        same = ddsp.ControlAlign(type("Conf", (), dict(sample_rate=SR)))(ctrl_a, ctrl_b, penalty=penalty)
        assert torch.equal(same[0], pos_a) and torch.equal(same[1], pos_b)


def test_argument_errors():
    xa, xb = torch.zeros(2, 5, 3), torch.zeros(2, 7, 3)
    for bad in (dict(radius=0), dict(radius=-1), dict(radius=1.5), dict(penalty=-0.1), dict(penalty=float("nan")), dict(penalty=float("inf")),
                dict(timing=float("nan")), dict(frames=0)):
        with pytest.raises(ValueError):
            ddsp.dtw_align(xa, xb, **bad)
    for other in (torch.zeros(3, 7, 3), torch.zeros(2, 7, 4), torch.zeros(2, 7), torch.zeros(2, 7, 3, device="meta"),
                  torch.zeros(2, 7, 3, dtype=torch.float64)):
        with pytest.raises(ValueError):
            ddsp.dtw_align(xa, other)
    with pytest.raises(RuntimeError, match="no backward"):      # refused as morph_controls refuses them
        ddsp.dtw_align(xa.requires_grad_(True), xb)
    empty = ddsp.dtw_align(torch.zeros(0, 5, 3), torch.zeros(0, 7, 3), return_path=True)
    assert [tuple(v.shape) for v in empty] == [(0, 5), (0, 5), (0, 11, 2), (0,), (0,)]
    A, _ = ref.phrase()
    ctrl = controls(A)
    bare = {k: v for k, v in ctrl.items() if k != "H"}
    with pytest.raises(ValueError, match="noise bands"):
        ddsp.align_controls(ctrl, bare, SR)
    with pytest.raises(ValueError, match="batch"):
        ddsp.align_controls(ctrl, {k: v.repeat(2, 1, 1) for k, v in ctrl.items()}, SR)
    with pytest.raises(ValueError):
        ddsp.align_controls(ctrl, {k: v.to("meta") for k, v in ctrl.items()}, SR)
    with pytest.raises(RuntimeError, match="no backward"):
        ddsp.align_controls(dict(ctrl, c=ctrl["c"].clone().requires_grad_(True)), ctrl, SR)
    with pytest.raises(ValueError):
        ddsp.control_features(ctrl, SR, n_bands=0)
    # the C entry answers before it touches the device
    L = ddsp._lib.lib()
    word = np.zeros(1, np.uint64)
    p = word.ctypes.data                                        # (a valid address; nothing is read from it)
    call = lambda **kw: L.ddsp_dtw_align(*[kw.get(k, p) for k in ("x_a", "x_b", "pos_a", "pos_b", "path", "length", "cost", "workspace")],  # noqa: E731
                                         kw.get("bytes", 1 << 40), kw.get("B", 1), kw.get("T_a", 4), kw.get("T_b", 4), kw.get("D", 2),
                                         kw.get("T_out", 4), kw.get("radius", 0), kw.get("penalty", 0.0), kw.get("timing", 0.0), None)
    EINVAL, ERANGE = -1, -2
    assert call(B=0) == 0
    for bad in (dict(x_a=None), dict(cost=None), dict(workspace=None), dict(B=-1), dict(T_a=0), dict(T_b=-3), dict(D=0), dict(T_out=0),
                dict(radius=-1), dict(penalty=-1.0), dict(penalty=float("nan")), dict(penalty=float("inf")), dict(timing=float("nan")),
                dict(timing=float("inf")), dict(bytes=0)):
        assert call(**bad) == EINVAL, bad
    for bad in (dict(T_a=analysis.DTW_KERNEL_MAX_FRAMES + 1), dict(T_b=analysis.DTW_KERNEL_MAX_FRAMES + 1),
                dict(D=analysis.DTW_KERNEL_MAX_FEATURES + 1), dict(B=2 ** 31), dict(T_out=2 ** 31)):
        assert call(**bad) == ERANGE, bad
    assert (analysis.DTW_KERNEL_MAX_FRAMES, analysis.DTW_KERNEL_MAX_FEATURES) == (ref.KERNEL_MAX_FRAMES, ref.KERNEL_MAX_FEATURES)
    assert L.ddsp_dtw_workspace_bytes(3, 65, 10) == 3 * 2 * 73 * 64 and L.ddsp_dtw_workspace_bytes(1, 2049, 1) == 0
    assert L.ddsp_dtw_workspace_bytes(0, 4, 4) == 0


def test_autoencoder_morph_refuses_positions_with_align():
    ae = ddsp.AutoEncoder(AEConf, tracker='yin')
    x = torch.zeros(1, AEConf.hop_length * 8)
    with pytest.raises(ValueError, match="align"):
        ae.morph(x, x, align=True, positions_a=torch.zeros(4))
