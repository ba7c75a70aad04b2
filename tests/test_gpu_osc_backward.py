"""The oscillator bank's backward (csrc/ddsp_osc_bwd.hip: osc_bwd_kernel<K, POW2> + osc_bwd_finish_kernel) against the fp64
reference of tests/osc_grad_reference.py, on every kernel variant: all nine K instantiations at G = 1, 4, 8, 16, both walks (POW2
and not), both grad_y paths (LDS and global memory), the exact-modulo walk, the Nyquist truncation of the walk, the finish
kernel's row and clip edges, the training shape and the reference's default config.

Every case asserts, elementwise, |grad_c - fp64| <= TOL * Yc[t] and |grad_a - fp64| <= TOL * Ya[t] (local yardsticks: a quiet
frame is held to its own scale, not the loudest one's), the same non-finite pattern as the reference, exact zeros above Nyquist
and in every batch row whose upstream gradient is zero, a bit-identical repeat, and the forward still <= 1e-5 of the loudness
around each sample against the oracle.  The per-family worst ratios are printed at the end of the module (pytest -s)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ddsp_pytorch_amd as ddsp  # noqa: E402
from ddsp_pytorch_amd import synthetic as syn  # noqa: E402
import fuzz_parity as fz  # noqa: E402

TOL = fz.OSC_BWD_TOL
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nosc backward, worst error / yardstick per family: " +
          ", ".join(f"{k} {v:.2e}" for k, v in sorted(WORST.items())))


class Conf:
    def __init__(self, n_harmonics, sample_rate, hop_length):
        self.n_harmonics, self.sample_rate, self.hop_length = n_harmonics, sample_rate, hop_length


def controls(B, T, H, hop, sr, seed, kind="musical", spread=True):
    ctl = syn.make_controls(syn.SynthShape("b", B, sr, hop, T, H, 2), seed, kind)
    rng = np.random.default_rng(seed + 7)
    if spread:                                              # loudness over seven decades from frame to frame
        ctl["a"] = ctl["a"] * (10.0 ** rng.uniform(-4, 3, size=ctl["a"].shape)).astype(np.float32)
    gy = rng.standard_normal((B, T * hop)).astype(np.float32)
    return ctl, gy


def check(r, family, K=None, G=None, quiet=False):
    WORST[family] = max(WORST.get(family, 0.0), r["rc"], r["ra"])
    if K is not None:
        assert r["K"] == K, r
    if G is not None:
        assert r["G"] == G, r
    assert r["rc"] <= TOL, r
    assert r["ra"] <= TOL, r
    assert r["nonfinite_same"], r
    assert r["masked_zero"], r
    assert r["quiet_zero"], r
    assert r["repeat_same"], r
    assert r["y_err"] <= 1e-5 and r["y_nonfinite_same"], r
    if quiet:
        assert r["quiet_rows"] >= 1, r


def one_loud_row(gy, b):
    """Upstream gradient in row b only: every other row's gradient must be exactly zero (no leak between rows)."""
    keep = gy[b].copy()
    gy[:] = 0.0
    gy[b] = keep
    return gy


# ---- every tiling: K x G, pinned through the tuning hook across the forward and the backward ----------------------------
TILINGS = [(K, G) for K in fz.OSC_KS for G in (1, 4, 8, 16)]
HOPS_CYCLE = [64, 3, 100, 2, 160, 7, 128, 48, 1]


def tiling_case(K, G):
    i = TILINGS.index((K, G))
    H = K if G == 1 else K * G // 2 + 1 + (i % (K * G // 2))
    hop = HOPS_CYCLE[i % len(HOPS_CYCLE)]
    T = 256 // G + 3                                        # two superblocks per row (NSB > 1), the second one ragged
    B = 3
    sr = [16000, 44100, 22050][i % 3]
    return B, T, H, hop, sr


@pytest.mark.parametrize("K,G", TILINGS)
def test_every_tiling(K, G):
    B, T, H, hop, sr = tiling_case(K, G)
    ctl, gy = controls(B, T, H, hop, sr, 100 + K * 17 + G, "musical" if G % 8 else "all_live")
    ctl["c"][:, :, (K + G) % H] = 0.0                       # an exactly-zero harmonic
    if G == 4:
        gy = one_loud_row(gy, 1)
    else:
        gy[2] = 0.0
    r = fz.osc_backward_case(ctl, gy, hop, sr, K=K)
    check(r, f"tiling K{K}", K=K, G=G, quiet=True)


# ---- the training shape (automatic tiling K=13, G=8) and the reference's default config (K=4, G=64) ----------------------
def test_training_shape_k13_g8():
    B, T, H, hop, sr = 32, 500, 100, 128, 16000           # cfg5's oscillator shape
    ctl, gy = controls(B, T, H, hop, sr, 5150)
    gy[7] = 0.0
    r = fz.osc_backward_case(ctl, gy, hop, sr, rows=[0, 7, 19, B - 1])
    check(r, "training K13 G8", K=13, G=8, quiet=True)


def test_reference_default_config_k4_g64():
    B, T, H, hop, sr = 2, 172, 180, 512, 44100
    ctl, gy = controls(B, T, H, hop, sr, 4410, spread=False)
    r = fz.osc_backward_case(ctl, gy, hop, sr)
    check(r, "default config K4 G64", K=4, G=64)


# ---- hops: the non-power-of-two walk (split_index, per-sample weights) and the power-of-two walk -------------------------
NPOW2_HOPS = [1, 3, 7, 48, 100, 160, 441, 480]
POW2_HOPS = [2, 64, 128, 256, 512, 1024, 2048]


@pytest.mark.parametrize("hop", NPOW2_HOPS + POW2_HOPS)
def test_hops(hop):
    sr = 44100 if hop in (441, 512, 2048) else 16000
    H = 40 if hop < 1024 else 12
    T = max(2, min(120, 1_500_000 // (2 * hop * H)))
    ctl, gy = controls(2, T, H, hop, sr, 900 + hop)
    if hop == 160:
        gy = one_loud_row(gy, 0)
    r = fz.osc_backward_case(ctl, gy, hop, sr)
    assert r["pow2"] == (hop in POW2_HOPS)
    check(r, "hop (pow2 walk)" if r["pow2"] else "hop (non-pow2 walk)", quiet=hop == 160)


def test_pow2_hop_past_2_23_samples_takes_the_general_walk():
    B, T, H, hop, sr = 1, 4097, 2, 2048, 16000              # T * hop = 2^23 + 2048: per-sample weights
    ctl, gy = controls(B, T, H, hop, sr, 4097)
    r = fz.osc_backward_case(ctl, gy, hop, sr)
    assert not r["pow2"] and not r["use_lds"]
    check(r, "hop (non-pow2 walk)")


# ---- grad_y through global memory (use_lds = 0) ------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,H,hop,K,G", [(1, 10, 60, 2048, 4, 16), (4, 40, 12, 1024, 4, 4), (3, 12, 30, 1600, None, None)])
def test_grad_y_in_global_memory(B, T, H, hop, K, G):
    ctl, gy = controls(B, T, H, hop, 16000, 70 + hop)
    if B > 2:
        gy = one_loud_row(gy, B - 1)
    r = fz.osc_backward_case(ctl, gy, hop, 16000)
    assert not r["use_lds"], r
    check(r, "grad_y global", K=K, G=G, quiet=B > 2)


# ---- the exact-modulo walk ----------------------------------------------------------------------------------------------
def test_exact_walk_negative_f0():
    ctl, gy = controls(2, 30, 24, 100, 16000, 81)
    ctl["f0"][1, 11, 0] = -150.0
    r = fz.osc_backward_case(ctl, gy, 100, 16000)
    assert r["exact"]
    check(r, "exact walk")


def test_exact_walk_huge_f0():
    ctl, gy = controls(3, 40, 60, 128, 16000, 82)
    ctl["f0"][2, :, 0] *= 300.0                             # masked harmonics at >= 1024 rad/sample
    gy = one_loud_row(gy, 2)
    r = fz.osc_backward_case(ctl, gy, 128, 16000)
    assert r["exact"]
    check(r, "exact walk", quiet=True)


def test_exact_walk_phase_past_1e7():
    B, T, H, hop, sr = 1, 4000, 2, 1024, 16000              # 4.1 M samples at ~3 rad/sample: the top harmonic passes 1e7 rad
    ctl, gy = controls(B, T, H, hop, sr, 83)
    ctl["f0"][:] = np.float32(0.47 * sr / 2)
    r = fz.osc_backward_case(ctl, gy, hop, sr)
    assert r["exact"]
    check(r, "exact walk")


# ---- the Nyquist truncation of the walk (KL = K/4, K/2, K) ---------------------------------------------------------------
@pytest.mark.parametrize("K,G,hop", [(4, 16, 64), (8, 8, 100), (13, 8, 128), (25, 4, 3), (16, 16, 48), (23, 1, 160)])
def test_nyquist_crossings(K, G, hop):
    sr = 16000
    H = K if G == 1 else K * G
    T = 64
    ctl, gy = controls(3, T, H, hop, sr, 300 + K)
    nyq = sr // 2
    # row 0: a glissando from every harmonic live to only the fundamental; row 1: f0 jumping between frames (a harmonic masked
    # at t but live at t +- 1); row 2: f0 exactly at Nyquist / k, so that harmonic k sits on Nyquist (kept: the mask is strict)
    ctl["f0"][0, :, 0] = np.geomspace(0.9 * nyq / H, 0.9 * nyq, T).astype(np.float32)
    rng = np.random.default_rng(K)
    ctl["f0"][1, :, 0] = np.exp(rng.uniform(np.log(nyq / H / 2), np.log(nyq), T)).astype(np.float32)
    ks = np.array([k for k in range(1, H + 1) if np.float32(k) * np.float32(nyq / k) == np.float32(nyq)])
    ctl["f0"][2, :, 0] = np.float32(nyq / ks[np.arange(T) % len(ks)])
    r = fz.osc_backward_case(ctl, gy, hop, sr, K=K)
    check(r, "nyquist crossings", K=K, G=G)


# ---- edges of the rows and the clip -------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,H,hop,sr", [(3, 1, 20, 64, 16000), (2, 1, 7, 441, 44100), (3, 2, 33, 100, 16000), (4, 2, 5, 2, 8000),
                                          (5, 7, 1, 160, 16000), (1, 300, 1, 3, 22050), (2, 9, 100, 128, 16000),
                                          (2, 13, 65, 7, 16000), (1, 8, 1600, 64, 48000), (7, 37, 50, 48, 16000)])
def test_edge_shapes(B, T, H, hop, sr):
    ctl, gy = controls(B, T, H, hop, sr, B * 1000 + T * 10 + H)
    if B > 2:
        gy = one_loud_row(gy, B // 2)
    r = fz.osc_backward_case(ctl, gy, hop, sr)
    check(r, "edges", quiet=B > 2)


@pytest.mark.parametrize("hop,sr", [(64, 16000), (100, 16000)])
def test_silent_frames_and_nan_f0(hop, sr):
    """Frames with S = 0 -- every c zero, or every harmonic above Nyquist -- give amp = 0/0 = NaN in the reference and on the
    device alike; a NaN-f0 frame between frames whose harmonics are all above Nyquist (the walk's truncation skips such slots);
    an exactly-zero harmonic; the NaN spreads along its row only."""
    B, T, H = 4, 40, 80
    ctl, gy = controls(B, T, H, hop, sr, 1234 + hop)
    ctl["c"][:, :, 5] = 0.0
    ctl["c"][0, 9, :] = 0.0                                # S = 0: every c zero
    ctl["f0"][1, 20, 0] = sr                               # S = 0: every harmonic above Nyquist
    ctl["f0"][2, 14:19, 0] = sr                            # ... around a NaN frame
    ctl["f0"][2, 16, 0] = np.nan
    ctl["f0"][2, 30:, 0] = sr
    r = fz.osc_backward_case(ctl, gy, hop, sr)
    check(r, "silent frames / NaN f0")


# ---- the module: autograd, autocast, and the chunked-form path hook -----------------------------------------------------
def module_grads(ctl, gy, hop, sr, autocast=False):
    B, T, H = ctl["c"].shape
    osc = ddsp.OscillatorBank(Conf(H, sr, hop)).cuda()
    c = torch.from_numpy(ctl["c"]).cuda().requires_grad_()
    a = torch.from_numpy(ctl["a"]).cuda().requires_grad_()
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        y = osc({"f0": torch.from_numpy(ctl["f0"]).cuda(), "c": c, "a": a})
    (y.float() * torch.from_numpy(gy).cuda()).sum().backward()
    torch.cuda.synchronize()
    return y.detach().float().cpu().numpy(), c.grad.cpu().numpy(), a.grad.cpu().numpy()


@pytest.mark.parametrize("B,T,H,hop,sr", [(2, 50, 100, 128, 16000), (3, 20, 24, 441, 44100), (2, 30, 180, 512, 44100)])
def test_module_autocast_equals_fp32_and_matches_fp64(B, T, H, hop, sr):
    ctl, gy = controls(B, T, H, hop, sr, 600 + hop)
    if B > 2:
        gy = one_loud_row(gy, 0)
    y, gc, ga = module_grads(ctl, gy, hop, sr)
    yb, gcb, gab = module_grads(ctl, gy, hop, sr, autocast=True)
    for u, v in ((y, yb), (gc, gcb), (ga, gab)):
        assert np.array_equal(fz.bits(u), fz.bits(v))
    r = fz.compare_osc_backward(ctl, gy, hop, sr, y, gc, ga)
    r.update(repeat_same=True)
    check(r, "module", quiet=B > 2)


def test_module_with_the_chunked_path_eligible_keeps_the_frame_scratch():
    """ddsp_osc_set_path(2) makes the chunked forward eligible at any batch; autograd still asks for the frame-form scratch the
    backward re-walks, and its gradients match fp64."""
    L = ddsp._lib.lib()
    B, T, H, hop, sr = 3, 60, 48, 128, 16000
    ctl, gy = controls(B, T, H, hop, sr, 77)
    try:
        ddsp._lib.check(L.ddsp_osc_set_path(2), "ddsp_osc_set_path")
        assert ddsp._lib.osc_plan(B, T, H, hop, sr)["chunked"] == 1
        y, gc, ga = module_grads(ctl, gy, hop, sr)
    finally:
        L.ddsp_osc_set_path(0)
    assert np.isfinite(gc).all() and np.isfinite(ga).all()
    r = fz.compare_osc_backward(ctl, gy, hop, sr, y, gc, ga)
    r.update(repeat_same=True)
    check(r, "module")


# ---- coverage: the cases above reach every variant of the backward kernel ----------------------------------------------
def test_cases_cover_every_kernel_variant():
    """From the case tables, by the launch's own selection (osc_plan under the same pinned tiling; pow2 / use_lds by the formulas of
    setup_params / launch_bwd): all nine K, both walks, both grad_y paths.  The exact walk is asserted by the three exact-walk
    tests from how their inputs were built (fz.osc_exact_walk_expected)."""
    L = ddsp._lib.lib()
    seen = set()
    for K, G in TILINGS:
        B, T, H, hop, sr = tiling_case(K, G)
        try:
            ddsp._lib.check(L.ddsp_osc_set_tiling(K), "ddsp_osc_set_tiling")
            k, g, pow2, lds = fz.osc_bwd_variant(B, T, H, hop, sr)
        finally:
            L.ddsp_osc_set_tiling(0)
        assert (k, g) == (K, G)
        seen |= {("K", k), ("pow2", pow2), ("lds", lds)}
    for B, T, H, hop in [(1, 10, 60, 2048), (4, 40, 12, 1024), (1, 4097, 2, 2048)]:
        k, g, pow2, lds = fz.osc_bwd_variant(B, T, H, hop, 16000)
        seen |= {("K", k), ("pow2", pow2), ("lds", lds)}
    assert {("K", k) for k in fz.OSC_KS} <= seen
    assert {("pow2", True), ("pow2", False), ("lds", True), ("lds", False)} <= seen
