"""CPU checks of the fp64 encoder-stage references (tests/encoder_reference.py) that tests/test_gpu_encoder_stages.py holds the HIP
kernels to: against the reference's own fixtures G19 / G20, and -- what makes the GPU tolerances fair -- that the stock fp32 CPU
branch stays within 1e-6 (loudness) and 5e-7 (resampler) of them on exactly the inputs the GPU tests use.  No GPU needed."""
import numpy as np
import pytest
import torch

import ddsp_pytorch_amd as ddsp
from conftest import load_golden
from encoder_common import loud_conf

import encoder_reference as R


def test_loudness_ref_matches_fixture_g19():
    g = load_golden("g19_loudness")
    for tag in ("a", "b"):
        conf = loud_conf(g, tag)
        ref = R.loudness_ref(g[f"{tag}_x"], conf.n_fft, conf.hop_length, g[f"{tag}_a_weight"])
        assert ref.shape == g[f"{tag}_loudness"].shape[:2]
        assert np.abs(ref - g[f"{tag}_loudness"][..., 0]).max() <= 2e-6, tag


def test_resample_ref_matches_fixture_g20():
    g = load_golden("g20_resample")
    for tag in ("a", "b"):
        ref = R.resample_ref(g[f"{tag}_x"], int(g[f"{tag}_rate"]), 16000)
        assert ref.shape == g[f"{tag}_y"].shape
        assert np.abs(ref - g[f"{tag}_y"]).max() <= 1e-6, tag
        some = np.array([0, 1, 17, ref.shape[1] - 1])
        assert np.array_equal(R.resample_ref(g[f"{tag}_x"], int(g[f"{tag}_rate"]), 16000, positions=some), ref[:, some])


@pytest.mark.parametrize("n_fft", R.LOUDNESS_SIZES)
def test_stock_fp32_loudness_stays_within_1e_6_on_the_gpu_tests_inputs(n_fft):
    aw = R.a_weight_of(n_fft)
    for c in R.loudness_cases(n_fft):
        enc = R.loudness_encoder(n_fft, c["hop"])
        assert np.array_equal(enc.a_weight.detach().numpy(), aw)
        ref = R.loudness_ref(c["x"], n_fft, c["hop"], aw)
        got = enc(torch.from_numpy(c["x"])).numpy()[..., 0].astype(np.float64)
        assert got.shape == ref.shape == c["nan_frames"].shape
        # the frames that hold the NaN / Inf sample, and only those, are lost in the stock path (NaN; an Inf sample gives NaN or
        # Inf, whichever the host's FFT code path makes of Inf * 0)
        assert np.array_equal(~np.isfinite(got), c["nan_frames"]) and np.array_equal(np.isnan(ref), c["nan_frames"]), c["name"]
        assert np.all(np.isnan(got[0][c["nan_frames"][0]]))
        ok = ~c["nan_frames"]
        err = np.abs(got - ref)[ok].max()
        assert err <= R.STOCK_LOUDNESS_TOL, (c["name"], err)
        if c["levels"] is not None and (c["levels"] == 0).any():
            assert np.all(np.abs(ref[c["levels"] == 0] + 3.45) < 0.05)      # digital silence: log10(1e-20) and the weights


def test_loudness_cases_place_quiet_frames_in_both_slots():
    for c in R.loudness_cases(64)[:2]:
        ratio = R.pair_ratio(c["levels"])
        for q in R.QUIET:
            quiet = np.isclose(ratio, q)
            assert quiet[0, 0::2].any() and quiet[1, 1::2].any()                  # slot a in row 0, slot b in row 1
        both = (c["levels"][2, 0:-1:2] < 1) & (c["levels"][2, 1::2] < 1)
        assert both.any()
    shapes = {(c["name"], c["x"].shape[0], c["nan_frames"].shape[1]) for c in R.loudness_cases(64)}
    assert {("steps9", 3, 9), ("steps8", 3, 8), ("one_frame", 3, 1)} <= shapes
    for n_fft in R.LOUDNESS_SIZES:
        nf = [c for c in R.loudness_cases(n_fft) if c["name"] == "non_finite"][0]
        dead = nf["nan_frames"]
        assert np.isnan(nf["x"][0]).sum() == 1 and np.isinf(nf["x"][1]).sum() == 1 and np.isfinite(nf["x"][2]).all()
        assert dead[0].sum() == 2 and dead[1].sum() == 2 and not dead[2].any()
        for row in (0, 1):                                     # the NaN row and the Inf row alike
            frames = [int(f) for f in np.nonzero(dead[row])[0]]
            assert {f & 1 for f in frames} == {0, 1}                             # either slot of a pair ...
            assert all(not dead[row, f ^ 1] for f in frames)                     # ... and each one's pair partner is live


@pytest.mark.parametrize("orig,new", R.RATE_PAIRS)
def test_stock_fp32_resampler_stays_within_5e_7_on_the_gpu_tests_inputs(orig, new):
    for L in R.resample_lengths(orig, new):
        x = R.resample_input(orig, new, L)
        ref = R.resample_ref(x, orig, new)
        got = R.stock_resample(x, orig, new)
        assert got.shape == ref.shape == (3, ddsp.encoder.resampled_length(L, orig, new))
        err = np.abs(got - ref).max()
        assert err <= R.STOCK_RESAMPLE_TOL, (L, err)


def test_stock_fp32_resampler_long_row_and_the_table_that_does_not_fit():
    orig, new = R.LONG_PAIR
    x = R.resample_input(orig, new, R.LONG_LENGTH, rows=1)
    got = R.stock_resample(x, orig, new)
    assert got.shape[1] > 16384 * 1024
    pos = R.long_positions(got.shape[1])
    assert pos.min() == 0 and pos.max() == got.shape[1] - 1 and pos.size == 3 * 4096
    assert np.abs(got[:, pos] - R.resample_ref(x, orig, new, positions=pos)).max() <= R.STOCK_RESAMPLE_TOL
    # 44056 -> 16000 reduces to 5507 : 2000: 2000 phase rows of 34 taps do not fit the kernel's 16384-float table
    table, _, K = ddsp.encoder.support_taps(44056, 16000)
    assert table.shape[0] * K > 16384
    x = R.resample_input(44056, 16000, 6000)
    assert np.abs(R.stock_resample(x, 44056, 16000) - R.resample_ref(x, 44056, 16000)).max() <= R.STOCK_RESAMPLE_TOL


def test_row_stats_frames_and_decode_references():
    rng = np.random.default_rng(5)
    y = (100.0 + 1e-3 * rng.standard_normal((2, 1500))).astype(np.float32)
    st = R.row_stats_ref(y)
    t = torch.from_numpy(y).double()
    assert np.allclose(st[:, 0], t.mean(1).numpy(), rtol=1e-15) and np.allclose(st[:, 1], t.std(1).numpy(), rtol=1e-12)
    fr = R.frames_fp32(y, st.astype(np.float32), 7, 3)
    assert fr.shape == (6, 1532) and fr.dtype == np.float32
    assert np.all(fr[:, :254] == 0) and np.all(fr[:, 1278:] == 0)
    want = (torch.from_numpy(y)[1, 14:14 + 1024] - np.float32(st[1, 0])) / np.float32(st[1, 1])
    assert np.array_equal(fr[5, 254:1278], want.numpy())
    const = R.frames_fp32(np.full((1, 1024), 3.0, np.float32), np.array([[3.0, 0.0]], np.float32), 1, 1)
    assert np.all(np.isnan(const[0, 254:1278])) and np.all(const[0, :254] == 0)
    z = (2.0 * rng.standard_normal((4, 360))).astype(np.float32)
    b = (0.1 * rng.standard_normal(360)).astype(np.float32)
    p = R.decode_ref(z, b)
    assert np.abs(p - torch.sigmoid(torch.from_numpy(z + b[None]).double()).numpy()).max() <= 1e-15
    z[0, 5], z[0, 6] = np.inf, -np.inf
    p = R.decode_ref(z, b)
    assert p[0, 5] == 1.0 and p[0, 6] == 0.0


def test_stock_fp32_stays_within_its_bounds_on_the_sweeps_cases():
    """The cases tests/test_gpu_fuzz.py draws (fuzz_parity.sweep_encoder_stages, seed 808)."""
    kinds = set()
    for c in R.sweep_cases(40, 808):
        kinds.add(c["kind"])
        if c["kind"] == "loudness":
            got = R.loudness_encoder(c["n_fft"], c["hop"])(torch.from_numpy(c["x"])).numpy()[..., 0]
            ref = R.loudness_ref(c["x"], c["n_fft"], c["hop"], R.a_weight_of(c["n_fft"]))
            tol = R.STOCK_LOUDNESS_TOL
        else:
            got, ref, tol = R.stock_resample(c["x"], c["orig"], c["new"]), R.resample_ref(c["x"], c["orig"], c["new"]), R.STOCK_RESAMPLE_TOL
        assert got.shape == ref.shape
        assert np.abs(got - ref).max() <= tol, (c["kind"], c.get("n_fft"), c.get("hop"), np.abs(got - ref).max())
    assert kinds == {"loudness", "resample"}


def test_resample_table_limit_is_the_kernels():
    """Resample chooses between the kernel and the stock ops by RESAMPLE_TABLE_MAX: it must be resample_kernel's LDS table size."""
    import os
    import re
    src = os.path.join(os.path.dirname(ddsp.__file__), "csrc", "ddsp_encoder.hip")
    if not os.path.exists(src):                                # the package is a module that re-exports ddsp-pytorch_amd/
        src = os.path.join(os.path.dirname(ddsp.encoder.__file__), "csrc", "ddsp_encoder.hip")
    with open(src) as f:
        m = re.search(r"constexpr int kMaxTable = (\d+);", f.read())
    assert m and int(m.group(1)) == ddsp.encoder.RESAMPLE_TABLE_MAX
    # one tap too many is refused before anything is launched (the pointers are never read)
    import ctypes
    buf = ctypes.create_string_buffer(16)
    p = ctypes.addressof(buf)
    assert ddsp._lib.lib().ddsp_resample(p, p, p, p, 1, 100, 3, ddsp.encoder.RESAMPLE_TABLE_MAX + 1, 1, None) == -2
    assert ddsp.encoder.Resample(16000, 16000).fits_kernel and ddsp.encoder.Resample(44100, 16000).fits_kernel
    assert not ddsp.encoder.Resample(44056, 16000).fits_kernel
