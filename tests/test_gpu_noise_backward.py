"""The filtered noise's backward (csrc/ddsp_noise.hip: ddsp_noise_backward_ws) against the fp64 reference of
tests/noise_grad_reference.py, on every kernel form it dispatches to:

    A  in-LDS FFT correlation (ddsp_noise_fft.hip: noise_fft_bwd_kernel<false>)       hop 512, S = 512, 16-byte aligned inputs
    B  FFT correlation -> dz, dH = dz C^T as a split-bf16 product (+ ddsp_noise_ir.hip)  hop 512, 193..224 bands, >= 512 frames
    C  batched direct kernel, 1 / 2 / 4 / 8 lanes per frame (noise_bwd_batched_kernel)    hop % 8 == 0 and the tile fits in LDS
    D  one frame per workgroup (noise_bwd_frame_kernel)                                   everything else, or mode bit 0

Every case asserts, elementwise, |dH - fp64| <= TOL * Y[f] (the frame's own yardstick: a quiet frame is held to its own scale,
not the loudest one's); per frame, max |err| <= 1e-5 * max |fp64| (exempt from this one only: frames whose gradient is below
1e-3 Y[f], and frames of 2 bands, whose whole gradient is one dot product that may cancel: fz.NOISE_BWD_FRAME_FLOOR); a bit-identical
repeat; exact zeros in frames whose upstream gradient is zero; and the non-finite contract: every dH of
a frame with a NaN / Inf upstream sample is non-finite, every other frame meets the contract -- except that forms A and B share
transforms between frames 2p and 2p + 1, so there the partner may come out entirely non-finite (never finite and wrong).  Every
case of forms A, B and C also runs under mode 1 (form D), which must meet the same contract and differ from the default bitwise
(the coverage guard: the default took another kernel; at 2 bands the batched kernel and form D evaluate the same fp32 sequence, so
there only the first holds).  The per-family worst ratios are printed at the end (pytest -s)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ddsp_pytorch_amd as ddsp  # noqa: E402
from ddsp_pytorch_amd import synthetic as syn  # noqa: E402
import fuzz_parity as fz  # noqa: E402
import noise_grad_reference as R  # noqa: E402
from oracle import oracle  # noqa: E402

TOL = fz.NOISE_BWD_TOL
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nnoise backward, worst error / yardstick per family: " +
          ", ".join(f"{k} {v:.2e}" for k, v in sorted(WORST.items())))


class Conf:
    def __init__(self, hop_length):
        self.n_harmonics, self.sample_rate, self.hop_length = 1, 16000, hop_length


def upstream(B, T, hop, seed, decades=True, zero=None):
    """grad_y [B, T*hop]: N(0,1) rows at per-frame levels 10^U(-4,3) (or ones); `zero`: (b, t) of a frame with no gradient."""
    rng = np.random.default_rng(seed)
    gy = rng.standard_normal((B, T, hop)).astype(np.float32) * fz.frame_levels(rng, B, T, decades)
    if zero is not None:
        gy[zero] = 0.0
    return gy.reshape(B, T * hop)


def uniform(B, T, hop, seed):
    return np.random.default_rng(seed + 1).random((B, T, hop), dtype=np.float32)


def check(r, family, form=None, zero=False, bad=0, frame_rel=fz.NOISE_BWD_FRAME_REL):
    WORST[family] = max(WORST.get(family, 0.0), r["ratio"], r.get("d_ratio", 0.0))
    if form is not None:
        assert r["form"] == form, r
    assert r["ratio"] <= TOL, r
    assert r["frame_rel"] <= frame_rel, r
    assert r["nonfinite_ok"], r
    assert r["bad_frames"] == bad, r
    assert r["zero_exact"], r
    assert r["repeat_same"], r
    if zero:
        assert r["zero_frames"] >= 1, r
    if r["form"] != "D" and "differs_from_d" in r:
        assert r["differs_from_d"] or r.get("F") == 2, r     # coverage guard: the default is not the one-frame-per-workgroup kernel
        assert r["d_ok"], r


# ---- A: in-LDS FFT correlation, 257 bands at hop 512 -------------------------------------------------------------------
PHILOX_OFFSET = 2**32 - 5          # the counters' low word carries inside the first frame of a launch


@pytest.mark.parametrize("B,T", [(1, 1), (3, 7), (3, 70)])
@pytest.mark.parametrize("draw", ["injected", "philox", "counter"])
def test_form_a(B, T, draw):
    F, hop = 257, 512
    gy = upstream(B, T, hop, 10 * B + T, zero=(B - 1, T // 2) if B * T > 1 else None)
    kw = dict(uniform=uniform(B, T, hop, T)) if draw == "injected" else dict(seed=0xDD5B0A7D, offset=PHILOX_OFFSET)
    if draw == "counter":
        kw["offset"] -= 3
        kw["counter"] = 5
    r = fz.noise_backward_case(gy, F, hop, same_as=2, **kw)
    check(r, "A fft", form="A", zero=B * T > 1)
    assert not r["same_as"], r                                # not the batched direct kernel either


# ---- B: the split-bf16 product, 193..224 bands at hop 512 from 512 frames ----------------------------------------------
@pytest.mark.parametrize("F", [194, 195, 223, 224])
@pytest.mark.parametrize("B,T", [(2, 256), (3, 171), (4, 150)])
def test_form_b(F, B, T):
    hop = 512
    assert ddsp._lib.lib().ddsp_noise_workspace_bytes(B, T, F, hop) > 0
    gy = upstream(B, T, hop, F + T, zero=(1, 17))
    kw = dict(uniform=uniform(B, T, hop, F)) if (F + T) % 2 else dict(seed=F, offset=(F << 40) + PHILOX_OFFSET)
    r = fz.noise_backward_case(gy, F, hop, same_as=2, **kw)
    check(r, "B product", form="B", zero=True)
    assert not r["same_as"], r                                # not the batched direct kernel either


def test_form_b_below_512_frames_and_mode_16_take_the_direct_kernels():
    """Observed on the device: bit-identical to the same call under mode 2, which forces the direct kernels."""
    F, hop = 195, 512
    assert ddsp._lib.lib().ddsp_noise_workspace_bytes(1, 511, F, hop) == 0
    gy = upstream(1, 511, hop, 511, zero=(0, 3))
    r = fz.noise_backward_case(gy, F, hop, seed=7, offset=PHILOX_OFFSET, against_d=False, same_as=2)
    check(r, "B declined", form="C3", zero=True)
    assert r["same_as"], r
    gy = upstream(4, 150, hop, 600, zero=(2, 3))
    r = fz.noise_backward_case(gy, F, hop, uniform=uniform(4, 150, hop, 600), mode=16, against_d=False, same_as=2)
    check(r, "B declined", form="C3", zero=True)
    assert r["same_as"], r


# ---- C: the batched direct kernel at every lane count (crop, pad, even F, F = 2; ragged last workgroups) ---------------
C_SHAPES = [(0, 2, 8, 1, 67), (0, 9, 16, 2, 33), (0, 65, 8, 3, 29), (0, 33, 40, 1, 100),
            (1, 65, 128, 3, 23), (1, 64, 128, 2, 35), (1, 129, 64, 1, 47),
            (2, 65, 160, 2, 9), (2, 128, 256, 3, 7), (2, 129, 256, 1, 17),
            (3, 101, 512, 2, 13), (3, 200, 480, 1, 11), (3, 257, 512, 3, 5), (3, 1025, 1024, 1, 9)]


@pytest.mark.parametrize("lpf,F,hop,B,T", C_SHAPES)
def test_form_c(lpf, F, hop, B, T):
    assert (B * T) % (64 >> lpf) != 0                       # a ragged last workgroup
    mode = 2 if (F, hop) == (257, 512) else 0               # (257 bands at hop 512 take form A by default)
    gy = upstream(B, T, hop, F * 1000 + hop, zero=(B - 1, T - 1))
    kw = dict(uniform=uniform(B, T, hop, F)) if lpf % 2 == 0 else dict(seed=F + hop, offset=PHILOX_OFFSET + F)
    r = fz.noise_backward_case(gy, F, hop, mode=mode, **kw)
    check(r, f"C lpf{lpf}", form=f"C{lpf}", zero=True)


# ---- D: one frame per workgroup ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,hop,B,T", [(9, 1, 2, 300), (5, 3, 2, 40), (33, 7, 3, 20), (65, 12, 2, 15), (33, 100, 3, 8),
                                       (129, 441, 2, 5), (1025, 2048, 1, 3)])
def test_form_d(F, hop, B, T):
    gy = upstream(B, T, hop, F * 10 + hop, zero=(0, 1))
    kw = dict(uniform=uniform(B, T, hop, hop)) if hop % 2 else dict(seed=hop, offset=PHILOX_OFFSET)
    r = fz.noise_backward_case(gy, F, hop, **kw)
    check(r, "D frame", form="D", zero=True)


@pytest.mark.parametrize("F,hop,B,T", [(64, 128, 2, 35), (33, 40, 1, 100)])
def test_form_d_under_mode_1(F, hop, B, T):
    gy = upstream(B, T, hop, F + hop, zero=(0, 2))
    r = fz.noise_backward_case(gy, F, hop, uniform=uniform(B, T, hop, 5), mode=1)
    check(r, "D frame", form="D", zero=True)


# ---- levels: 2^-110 and 2^90 next to a unit row (form A's equaliser clamps its exponent to +-100) ------------------------
# Below 2^-100 form A's equaliser stops at 2^100: a frame at 2^-110 paired with a unit row is scaled to 2^-10, not to [0.5, 1), and
# carries its partner's rounding 2^10 times larger relative to its own gradient (measured 1.4e-5 of its largest
# gradient, 1.6e-7 of its yardstick): held per frame to 4e-5, about 3x the measurement.  At 2^-100 the scaling is still exact.
CLAMP_ALLOWANCE = {2.0 ** -110: 4.0, 2.0 ** -100: 1.0}


def extreme_rows(B, T, hop, seed, lo, hi):
    gy = upstream(B, T, hop, seed, decades=False).reshape(B * T, hop)
    gy[0] *= np.float32(lo)                                  # frames 0 / 1 and 2 / 3: one transform pair each in form A
    gy[3] *= np.float32(hi)
    gy[5] *= np.float32(lo)
    return gy.reshape(B, T * hop)


@pytest.mark.parametrize("F,hop,mode,form,lo", [(257, 512, 0, "A", 2.0 ** -110), (257, 512, 0, "A", 2.0 ** -100),
                                                (257, 512, 2, "C3", 2.0 ** -110), (65, 128, 0, "C1", 2.0 ** -110),
                                                (9, 16, 0, "C0", 2.0 ** -110), (33, 100, 0, "D", 2.0 ** -110), (129, 441, 0, "D", 2.0 ** -110)])
def test_extreme_levels(F, hop, mode, form, lo):
    B, T = 1, 7
    gy = extreme_rows(B, T, hop, F + hop, lo, 2.0 ** 90)
    r = fz.noise_backward_case(gy, F, hop, uniform=uniform(B, T, hop, 3), mode=mode)
    allowance = CLAMP_ALLOWANCE[lo] if form == "A" else 1.0
    check(r, f"levels 2^{int(np.log2(lo))} / 2^90 {form}", form=form, frame_rel=fz.NOISE_BWD_FRAME_REL * allowance)


@pytest.mark.parametrize("F", [195, 224])
def test_form_b_levels_2_pm_60(F):
    """The split-bf16 product keeps its three terms normal at 2^+-60 of a unit row (the level below which the
    lowest term leaves the normal range)."""
    B, T, hop = 2, 260, 512
    gy = extreme_rows(B, T, hop, F, 2.0 ** -60, 2.0 ** 60)
    r = fz.noise_backward_case(gy, F, hop, seed=3, offset=PHILOX_OFFSET)
    check(r, "B product", form="B")


# ---- alignment: 4-byte-offset views make forms A and B decline to the direct kernels ------------------------------------
@pytest.mark.parametrize("F,B,T,form", [(257, 3, 7, "C3"), (195, 2, 256, "C3"), (224, 4, 150, "C3")])
@pytest.mark.parametrize("which", [("grad_y",), ("uniform",), ("grad_y", "uniform")])
def test_misaligned_inputs(F, B, T, form, which):
    hop = 512
    gy = upstream(B, T, hop, F + B)
    if which == ("grad_y",):
        r = fz.noise_backward_case(gy, F, hop, seed=F, offset=PHILOX_OFFSET, misalign=which, same_as=2)
    else:
        r = fz.noise_backward_case(gy, F, hop, uniform=uniform(B, T, hop, F), misalign=which, same_as=2)
    check(r, "misaligned", form=form)
    assert r["same_as"], r                                    # declined on the device: the direct kernels' very bits


# ---- non-finite upstream gradients ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,hop,B,T,mode,form", [(257, 512, 3, 7, 0, "A"), (195, 512, 3, 171, 0, "B"), (65, 128, 2, 35, 0, "C1"),
                                                 (9, 16, 1, 67, 0, "C0"), (257, 512, 3, 7, 2, "C3"), (33, 100, 3, 8, 0, "D"),
                                                 (65, 7, 2, 9, 0, "D")])
def test_non_finite_upstream_gradient(F, hop, B, T, mode, form):
    gy = upstream(B, T, hop, F * 3 + hop).reshape(B * T, hop)
    n = B * T
    gy[4, hop // 3] = np.nan                                  # frame 4: partner 5 in the paired forms
    gy[9, 0] = np.inf                                         # the first sample: only lag 0 sees it
    gy[n - 1, hop - 1] = -np.inf                              # the last sample of the last frame: every lag sees it
    gy = gy.reshape(B, T * hop)
    r = fz.noise_backward_case(gy, F, hop, uniform=uniform(B, T, hop, 9), mode=mode)
    check(r, f"non-finite {form[0]}", form=form, bad=3)


@pytest.mark.parametrize("F,hop,B,T,mode,paired", [(65, 128, 2, 20, 0, False), (257, 512, 3, 7, 0, True), (33, 64, 2, 9, 0, False),
                                                   (33, 100, 2, 9, 0, False), (195, 512, 1, 6, 0, True)])
def test_forward_non_finite_magnitudes(F, hop, B, T, mode, paired):
    """The same contract forward: NaN in one frame's H makes that frame's audio non-finite (the oracle's is), every other frame
    within 2e-6 of its peak -- across the wave form (hop 128 / 65 bands, whole groups of 16 frames), the FFT form (hop 512, where
    the pair partner may come out entirely non-finite) and the direct forms."""
    rng = np.random.default_rng(F + hop)
    Hm = syn.controller_range(rng.standard_normal((B, T, F), dtype=np.float32))
    Hm[B - 1, 5, F // 3] = np.nan
    u = uniform(B, T, hop, 2)
    ref = oracle.noise_forward(Hm, u, hop).reshape(B * T, hop)
    got = ddsp.noise_forward(torch.from_numpy(Hm).cuda(), hop, uniform=torch.from_numpy(u).cuda()).cpu().numpy().reshape(B * T, hop)
    bad = np.zeros(B * T, bool)
    bad[(B - 1) * T + 5] = True
    assert (~np.isfinite(ref[bad])).all() and np.isfinite(ref[~bad]).all()
    assert (~np.isfinite(got[bad])).all()
    ok = ~bad
    if paired:
        partner = (B - 1) * T + 5 ^ 1
        if not np.isfinite(got[partner]).any():
            ok[partner] = False
    assert np.isfinite(got[ok]).all()
    peak = np.maximum(np.abs(ref[ok]).max(axis=1), 1e-30)
    assert (np.abs(got[ok] - ref[ok]).max(axis=1) <= 2e-6 * peak).all()


# ---- the module: autograd with the in-kernel draw over two successive calls, and bf16 autocast ---------------------------
@pytest.mark.parametrize("F,hop,B,T", [(65, 128, 2, 40), (257, 512, 2, 9), (195, 512, 2, 300)])
def test_module_device_draw_two_calls(F, hop, B, T):
    fn = ddsp.FilteredNoise(Conf(hop), rng="device", seed=0xC0FFEE)
    fn.reseed(0xC0FFEE, PHILOX_OFFSET)
    rng = np.random.default_rng(F)
    for call in range(2):
        offset = fn._offset
        assert offset == PHILOX_OFFSET + call * fn.draws(B, T)
        H = torch.from_numpy(syn.controller_range(rng.standard_normal((B, T, F), dtype=np.float32))).cuda().requires_grad_()
        gy = upstream(B, T, hop, 100 * call + F)
        y = fn({"H": H})
        (y * torch.from_numpy(gy).cuda()).sum().backward()
        got = H.grad.cpu().numpy()
        ref, Y = R.noise_grad_fp64(gy, F, hop, seed=0xC0FFEE, offset=offset)
        r = fz.compare_noise_backward(got, ref, Y, gy, hop)
        r.update(repeat_same=True, form=fz.noise_bwd_form(B, T, F, hop))
        check(r, "module")


@pytest.mark.parametrize("F,hop,B,T", [(65, 128, 2, 40), (257, 512, 1, 9), (33, 100, 2, 7)])
def test_module_bf16_autocast(F, hop, B, T):
    """A bf16 leaf under autocast: the forward runs in fp32 (custom_fwd casts), the leaf's gradient is the fp32 gradient cast to
    bf16 -- bit-identical to that cast of the fp32 run, and within one bf16 ulp (plus the fp32 contract) of the fp64 reference."""
    rng = np.random.default_rng(F + 1)
    Hb = torch.from_numpy(syn.controller_range(rng.standard_normal((B, T, F), dtype=np.float32))).to(torch.bfloat16)
    u = uniform(B, T, hop, 4)
    gy = upstream(B, T, hop, F + 2)
    fn = ddsp.FilteredNoise(Conf(hop))

    def grad(autocast):
        H = Hb.cuda().clone().requires_grad_() if autocast else Hb.float().cuda().requires_grad_()
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            y = fn({"H": H}, noise=torch.from_numpy(u).cuda())
        (y.float() * torch.from_numpy(gy).cuda()).sum().backward()
        return H.grad

    g32, gbf = grad(False), grad(True)
    assert gbf.dtype == torch.bfloat16
    assert torch.equal(gbf, g32.to(torch.bfloat16))
    ref, Y = R.noise_grad_fp64(gy, F, hop, uniform=u)
    r = fz.compare_noise_backward(g32.cpu().numpy(), ref, Y, gy, hop)
    r.update(repeat_same=True, form=fz.noise_bwd_form(B, T, F, hop))
    check(r, "module")
    refb = torch.from_numpy(ref).to(torch.bfloat16).double()
    ulp = torch.from_numpy(np.spacing(np.abs(ref).astype(np.float32))).double() * 2.0 ** 16      # bf16: 16 fewer mantissa bits
    slack = ulp + TOL * torch.from_numpy(Y)[..., None]
    assert ((gbf.double().cpu() - refb).abs() <= slack).all()


# ---- argument checks before any launch ------------------------------------------------------------------------------------
def test_backward_rejects_bad_arguments_before_launching():
    B, T, hop, F = 2, 3, 16, 9
    g = torch.zeros(B, T * hop, device="cuda")
    with pytest.raises(ValueError):
        ddsp.noise_backward(torch.zeros(B, T, hop, device="cuda"), hop, F)            # not 2-D
    with pytest.raises(ValueError):
        ddsp.noise_backward(torch.zeros(B, T * hop + 4, device="cuda"), hop, F)       # width not a multiple of hop
    with pytest.raises(ValueError):
        ddsp.noise_backward(g, hop, 1)                                                # n_filters < 2
    with pytest.raises(ValueError):
        ddsp.noise_backward(g, hop, F, uniform=torch.zeros(B, T, hop + 4, device="cuda"))
    with pytest.raises(ValueError):
        ddsp.noise_backward(g, hop, F, uniform=torch.zeros(B, T + 1, hop, device="cuda"))
    with pytest.raises(ValueError):
        ddsp.noise_backward(g, hop, F, uniform=torch.zeros(B, T, hop, device="cuda", dtype=torch.float64))
    with pytest.raises(ValueError):
        ddsp.noise_backward(g, hop, F, counter=torch.zeros(1, device="cuda", dtype=torch.int32))
    with pytest.raises(ValueError):
        ddsp.noise_backward(g, hop, F, counter=torch.zeros(2, device="cuda", dtype=torch.int64))
    with pytest.raises(ValueError):
        ddsp.noise_backward(g, hop, F, uniform=torch.zeros(B, T, hop, device="cuda"),
                            counter=torch.zeros(1, device="cuda", dtype=torch.int64))
    assert ddsp.noise_backward(g, hop, F).shape == (B, T, F)                         # the good call still runs


def test_shape_beyond_the_frame_kernels_lds_is_reported():
    """4097 bands at hop 16384: no batched tile fits and the one-frame kernels need more than 160 KiB of LDS; both directions
    return DDSP_ERANGE before any launch."""
    F, hop = 4097, 16384
    with pytest.raises(ddsp._lib.DdspHipError, match="DDSP_ERANGE"):
        ddsp.noise_forward(torch.ones(1, 1, F, device="cuda"), hop, seed=1)
    with pytest.raises(ddsp._lib.DdspHipError, match="DDSP_ERANGE"):
        ddsp.noise_backward(torch.ones(1, hop, device="cuda"), hop, F, seed=1)
