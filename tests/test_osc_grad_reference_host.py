"""CPU checks of the fp64 oscillator-gradient reference (tests/osc_grad_reference.py) that tests/test_gpu_osc_backward.py
holds the HIP backward to: against the reference-autograd fixture G10, against autograd of the fp32 torch restatement, against
fp64 central differences, and that its local yardsticks bound the terms they claim to bound.  No GPU needed."""
import numpy as np
import pytest
import torch

from conftest import load_golden

import osc_grad_reference as R
from ddsp_pytorch_amd import synthetic as syn
from oracle import torch_restatement as tr


def test_matches_the_reference_autograd_fixture_g10():
    g = load_golden("g10_osc_grad")
    y, gc, ga, Yc, Ya = R.osc_grad_fp64(g["f0"], g["c"], g["a"], g["g"], int(g["hop"]), int(g["sample_rate"]))
    assert np.max(np.abs(y - g["y"])) <= 1e-6
    assert np.max(np.abs(gc - g["grad_c"])) <= 1e-6 * np.max(np.abs(g["grad_c"]))
    assert np.max(np.abs(ga - g["grad_a"])) <= 1e-6 * np.max(np.abs(g["grad_a"]))


@pytest.mark.parametrize("T,hop,frames", [(50, 441, (0, 1, 25, 49)), (9, 1, (0, 4, 8)), (4097, 2048, (0, 4090, 4095, 4096))])
def test_interpolation_is_the_fp32_f_interpolate(T, hop, frames):
    """`up` has the weights and the bracketing frames of the reference's fp32 F.interpolate, also past 2^23 samples (4097 x 2048),
    where i + 0.5 rounds in fp32: each column of the upsampled identity, i.e. w(i, t) of every sample for frame t."""
    br = R.brackets(T, hop)
    for t in frames:
        e = torch.zeros(T, 1, dtype=torch.float64)
        e[t] = 1.0
        ref = torch.nn.functional.interpolate(e.float().T[None], scale_factor=hop, mode="linear")[0, 0].double()
        assert float((R.up(e, br)[:, 0] - ref).abs().max()) <= 6e-8
        assert torch.equal(R.up(e, br)[:, 0] != 0, ref != 0)


def _controls(B, T, H, hop, sr, seed, kind="musical"):
    ctl = syn.make_controls(syn.SynthShape("r", B, sr, hop, T, H, 2), seed, kind)
    rng = np.random.default_rng(seed + 1)
    ctl["a"] = ctl["a"] * (10.0 ** rng.uniform(-4, 3, size=ctl["a"].shape)).astype(np.float32)   # seven decades
    gy = rng.standard_normal((B, T * hop)).astype(np.float32)
    return ctl, gy


def _nyquist_controls():
    # 16 kHz: f0 = 500 puts harmonic 16 exactly at Nyquist (kept: the mask is strict), f0 = 1000 masks 8..24, and a
    # glissando masks a changing number of harmonics from frame to frame
    ctl, gy = _controls(2, 12, 24, 64, 16000, 31)
    ctl["f0"][0, :, 0] = 500.0
    ctl["f0"][0, 3, 0] = 1000.0
    ctl["f0"][1, :, 0] = np.geomspace(200.0, 4000.0, 12).astype(np.float32)
    return ctl, gy, 64, 16000


@pytest.mark.parametrize("case", ["hop441", "hop1", "nyquist"])
def test_fp32_restatement_autograd_is_within_1e6_of_the_yardsticks(case):
    if case == "hop441":
        ctl, gy = _controls(2, 9, 40, 441, 44100, 5)
        hop, sr = 441, 44100
    elif case == "hop1":
        ctl, gy = _controls(2, 300, 30, 1, 16000, 6, "all_live")
        ctl["f0"][1, ::7, 0] = 3000.0                       # masked harmonics on every seventh frame
        hop, sr = 1, 16000
    else:
        ctl, gy, hop, sr = _nyquist_controls()
    _, gc, ga, Yc, Ya = R.osc_grad_fp64(ctl["f0"], ctl["c"], ctl["a"], gy, hop, sr)
    c32 = torch.from_numpy(ctl["c"]).requires_grad_()
    a32 = torch.from_numpy(ctl["a"]).requires_grad_()
    y32 = tr.oscillator_bank(torch.from_numpy(ctl["f0"]), c32, a32, hop, sr)
    (y32 * torch.from_numpy(gy)).sum().backward()
    assert np.isfinite(gc).all() and np.isfinite(ga).all()
    rc, ra = R.ratio(c32.grad.numpy(), gc, Yc), R.ratio(a32.grad.numpy(), ga, Ya)
    assert rc <= 1e-6 and ra <= 1e-6, (rc, ra)
    mask = R.harmonic_mask(ctl["f0"].reshape(-1, 1), ctl["c"].shape[-1], sr).numpy().reshape(gc.shape)
    assert mask.any() or case == "hop441"
    assert (gc[mask] == 0.0).all()
    if case == "nyquist":
        assert not mask[0, 0, 15] and mask[0, 0, 16]        # harmonic 16 at exactly 8 kHz is live, 17 is not


def test_central_differences():
    ctl, gy, hop, sr = _nyquist_controls()
    _, gc, ga, _, _ = R.osc_grad_fp64(ctl["f0"], ctl["c"], ctl["a"], gy, hop, sr)
    b = 1
    phi, _ = R.row_phases(ctl["f0"], ctl["c"], ctl["a"], b, hop, sr)
    T, H = ctl["c"].shape[1:]
    br = R.brackets(T, hop)
    mask = R.harmonic_mask(ctl["f0"][b], H, sr)
    g = torch.from_numpy(gy[b]).double()
    c0 = torch.from_numpy(ctl["c"][b]).double()
    a0 = torch.from_numpy(ctl["a"][b]).double()
    assert torch.isfinite(R.row_output(c0, a0, mask, phi, br)).all()

    def dloss(cp, ap, cm, am):
        # sum_i (y+ - y-)_i g_i: the samples the entry does not reach cancel exactly, not against the whole clip's loss
        return float(((R.row_output(cp, ap, mask, phi, br) - R.row_output(cm, am, mask, phi, br)) * g).sum())

    masked = [(t, k) for t in range(T) for k in range(H) if mask[t, k]]
    assert masked
    for t, k in [(0, 0), (5, 3), (T - 1, 1), masked[0], masked[-1]]:
        h = 1e-6 * float(c0[t, k])
        cp, cm = c0.clone(), c0.clone()
        cp[t, k] += h
        cm[t, k] -= h
        fd = dloss(cp, a0, cm, a0) / (2 * h)
        if mask[t, k]:
            assert fd == 0.0 and gc[b, t, k] == 0.0
        else:
            assert abs(fd - gc[b, t, k]) <= 1e-6 * max(abs(gc[b, t, k]), 1e-3 * float(np.abs(gc[b]).max())), (t, k, fd, gc[b, t, k])
    for t in (0, 6, T - 1):
        h = 1e-6 * float(a0[t, 0])
        ap, am = a0.clone(), a0.clone()
        ap[t, 0] += h
        am[t, 0] -= h
        fd = dloss(c0, ap, c0, am) / (2 * h)
        assert abs(fd - ga[b, t, 0]) <= 1e-7 * float(np.abs(ga[b]).max()), (t, fd, ga[b, t, 0])


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_yardsticks_bound_the_terms(seed):
    rng = np.random.default_rng(seed)
    hop = int(rng.choice([1, 3, 64, 100, 441]))
    sr = int(rng.choice([16000, 44100]))
    T, H, B = int(rng.integers(1, 30)), int(rng.integers(1, 50)), 2
    ctl, gy = _controls(B, T, H, hop, sr, seed + 10)
    ctl["c"][:, :, rng.integers(0, H)] = 0.0
    _, gc, ga, Yc, Ya = R.osc_grad_fp64(ctl["f0"], ctl["c"], ctl["a"], gy, hop, sr)
    assert (np.abs(gc) <= Yc[..., None]).all()
    assert (np.abs(ga[..., 0]) <= Ya).all()
