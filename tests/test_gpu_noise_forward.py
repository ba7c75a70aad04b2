"""The filtered noise's forward (csrc/ddsp_noise.hip: ddsp_noise_forward_ws) against the fp64 reference of
tests/noise_fwd_reference.py, on every kernel form it dispatches to (fuzz_parity.noise_fwd_form names them):

    FFT      in-LDS FFT form (ddsp_noise_fft.hip): hop 512 -- one packed inverse FFT at 257 bands, cosine sums otherwise -- and, under
             mode 4, hop 256; two frames share every transform
    FFT+IR   the same, its impulse responses from the whole-batch split-bf16 product (ddsp_noise_ir.hip): 193..224 bands, >= 4 096 frames
    WAVE     wavefront-private form (ddsp_noise_wave.hip): hop 128 / 65 bands, whole groups of 16 frames; WAVE+Cl: the remainder
    C0..C3   batched direct kernel, 64 >> l frames per workgroup (noise_batched_kernel)
    D        one frame per workgroup (noise_frame_kernel): everything else, a misaligned output, or mode bit 0

H is controller_range(N(0,1)) at per-frame levels 10^U(-4,3), with one exactly-zero frame wherever there is more than one frame, so
that a quiet frame is held to its own scale.  Every case asserts the form the Python mirror of the planner names; per sample
|y - fp64| <= TOL_SAMPLE * Y[n] (the direct forms: C, D, WAVE); per frame max |err| <= TOL_FRAME * Yframe (every form) and
max |err| <= FRAME_REL * the frame's own fp64 peak; exact zeros in frames whose H is zero; a bit-identical repeat; an output
pre-filled with NaN fully overwritten.  Every case of another form also runs under mode 1 (form D), which must meet the same contract and differ from the default bitwise (the coverage guard: at 2 bands the batched kernel
and form D evaluate the same fp32 sequence, so there only the first holds).  The tolerances are derived on the host
(tests/test_noise_fwd_reference_host.py::test_device_bounds), none is read off the device.  The worst figures per family are printed
at the end (pytest -s)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ddsp_pytorch_amd as ddsp  # noqa: E402
import fuzz_parity as fz  # noqa: E402
import noise_fwd_reference as R  # noqa: E402

WORST = {}
PHILOX_OFFSET = 2**32 - 5          # the counters' low word carries inside the first frame of a launch


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nnoise forward, worst (error / Y[n] per sample, error / Yframe, error / the frame's peak) per family: " +
          ", ".join(f"{k} ({v[0]:.2e}, {v[1]:.2e}, {v[2]:.2e})" for k, v in sorted(WORST.items())))


def draw(B, T, hop, key, kind=None):
    """Alternately the injected draw and the in-kernel one at PHILOX_OFFSET; kind 'counter': the offset split with a device counter."""
    kind = kind or ("injected" if key % 2 == 0 else "philox")
    if kind == "injected":
        return dict(uniform=R.gpu_uniform(B, T, hop, key))
    kw = dict(seed=0xDD5B0A7D + key, offset=PHILOX_OFFSET)
    if kind == "counter":
        kw.update(offset=PHILOX_OFFSET - 3, counter=5)
    return kw


def check(r, form, label=None, zero=True, bad=0):
    for fam, fig in r["parts"].items():
        key = fam if label is None else f"{label} {fam}"
        WORST[key] = tuple(max(a, b) for a, b in zip(WORST.get(key, (0.0, 0.0, 0.0)), fig))
    print(f"\n{form}{'' if label is None else ' (' + label + ')'}: {r}")
    assert r["form"] == form, r
    if r["direct"]:
        assert r["ratio_sample"] <= R.TOL_SAMPLE, r
    assert r["ratio_frame"] <= R.TOL_FRAME, r
    assert r["frame_rel"] <= R.FRAME_REL, r
    assert r["exempt_frames"] == 0, r
    assert r["nonfinite_ok"], r
    assert r["bad_frames"] == bad, r
    assert r["zero_exact"], r
    assert r["repeat_same"], r
    if zero:
        assert r["zero_frames"] >= 1, r
    if "differs_from_d" in r:
        assert r["differs_from_d"] or r["F"] == 2, r          # coverage guard: the default is not the one-frame-per-workgroup kernel
        assert r["d_ok"], r


# ---- FFT: hop 512, cosine sums (and the packed inverse FFT at 257 bands) ---------------------------------------------------
@pytest.mark.parametrize("F", [257, 195, 129, 256, 3])        # S = hop, the default shape, a zero gap, S = 510 (no power of two), S = 4
@pytest.mark.parametrize("B,T", [(1, 1), (3, 7), (3, 21)])    # odd frame counts: the last pair is half empty
def test_fft_form(F, B, T):
    hop = 512
    H = R.gpu_H(B, T, F, 1000 * F + T)
    kind = "counter" if (F, T) in ((257, 7), (195, 21)) else None
    r = fz.noise_forward_case(H, hop, same_as=2, **draw(B, T, hop, F + T, kind))
    check(r, "FFT", zero=B * T > 1)
    assert not r["same_as"], r                                # not the batched direct kernel either


@pytest.mark.parametrize("F", [129, 100, 65])
def test_fft_form_at_hop_256(F):
    B, T, hop = 3, 7, 256
    H = R.gpu_H(B, T, F, 256 + F)
    r = fz.noise_forward_case(H, hop, mode=4, same_as=0, **draw(B, T, hop, F))
    check(r, "FFT", label="hop 256")
    assert not r["same_as"], r                                # the default mode takes the batched kernel there


# ---- FFT + matrix product: 193..224 bands from 4 096 frames ----------------------------------------------------------------
@pytest.mark.parametrize("F,B,T", [(193, 1, 4097), (195, 3, 1399), (224, 1, 4097)])
def test_fft_form_with_the_matrix_product(F, B, T):
    hop = 512
    assert ddsp._lib.lib().ddsp_noise_workspace_bytes(B, T, F, hop) > 0
    H = R.gpu_H(B, T, F, F + T)
    r = fz.noise_forward_case(H, hop, against_d=False, same_as=16, **draw(B, T, hop, F))
    check(r, "FFT+IR")
    assert not r["same_as"], r                                # mode 16: the cosine sums -- another kernel's bits
    assert fz.noise_fwd_form(B, T, F, hop, mode=16) == "FFT"


def test_the_matrix_product_declines_below_4096_frames():
    F, B, T, hop = 195, 1, 4095, 512
    assert ddsp._lib.lib().ddsp_noise_workspace_bytes(B, T, F, hop) > 0          # (the backward's product starts at 512 frames)
    H = R.gpu_H(B, T, F, 4095)
    r = fz.noise_forward_case(H, hop, against_d=False, same_as=16, **draw(B, T, hop, 1))
    check(r, "FFT", label="product declined")
    assert r["same_as"], r                                    # declined on the host: the cosine sums' very bits


# ---- WAVE: hop 128 / 65 bands ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T", [(1, 16), (1, 17), (3, 11), (2, 40)])      # (2, 40): a row boundary inside a group of 16
def test_wave_form(B, T):
    F, hop = 65, 128
    H = R.gpu_H(B, T, F, 128 + T)
    kind = "counter" if T == 17 else None
    r = fz.noise_forward_case(H, hop, same_as=8, **draw(B, T, hop, T, kind))
    check(r, "WAVE" if (B * T) % 16 == 0 else "WAVE+C1")
    assert not r["same_as"], r                                # mode 8: the batched kernel on every frame


def test_wave_form_with_more_groups_than_wavefronts():
    """The persistent grid holds residency x CUs wavefronts; one more group of 16 frames than that, so that at least one wavefront
    takes a second group (and 5 frames more for the remainder)."""
    F, hop = 65, 128
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    groups = ddsp._lib.lib().ddsp_noise_get_residency() * cus + 1
    B, T = 1, 16 * groups + 5
    H = R.gpu_H(B, T, F, 77)
    r = fz.noise_forward_case(H, hop, against_d=False, same_as=8, seed=77, offset=PHILOX_OFFSET)
    check(r, "WAVE+C1", label="persistent")
    assert not r["same_as"], r


# ---- C: the batched direct kernel at every lane count (crop, pad, even F, F = 2; ragged last workgroups) -----------------------
C_SHAPES = [(0, 2, 8, 1, 67), (0, 9, 16, 2, 33), (0, 65, 8, 3, 29), (0, 33, 40, 1, 100),
            (1, 64, 128, 2, 35), (1, 129, 64, 1, 47),
            (2, 65, 160, 2, 9), (2, 129, 256, 1, 17), (2, 128, 256, 3, 7), (2, 1025, 1024, 1, 9),
            (3, 101, 512, 2, 13), (3, 257, 512, 3, 5), (3, 195, 512, 2, 9)]


@pytest.mark.parametrize("lpf,F,hop,B,T", C_SHAPES)
def test_batched_form_natural_lane_counts(lpf, F, hop, B, T):
    assert (B * T) % (64 >> lpf) != 0                         # a ragged last workgroup
    mode = 2 if hop == 512 and 2 * (F - 1) <= hop else 0      # (these take the FFT form by default)
    H = R.gpu_H(B, T, F, F * 1000 + hop)
    r = fz.noise_forward_case(H, hop, mode=mode, **draw(B, T, hop, F + lpf))
    check(r, f"C{lpf}")


@pytest.mark.parametrize("lpf", [0, 1, 2, 3])
@pytest.mark.parametrize("F,hop,B,T", [(65, 128, 2, 35), (9, 16, 2, 33), (129, 256, 1, 17), (33, 8, 1, 67)])
def test_batched_form_forced_lane_counts(lpf, F, hop, B, T):
    assert (B * T) % (64 >> lpf) != 0
    mode = ((lpf + 1) << 8) | 8                               # (bit 3: hop 128 / 65 bands stays out of the wavefront form)
    H = R.gpu_H(B, T, F, F * 100 + hop + lpf)
    r = fz.noise_forward_case(H, hop, mode=mode, **draw(B, T, hop, F + lpf + 1))
    check(r, f"C{lpf}", label="forced")


def test_wave_remainder_at_forced_lane_counts():
    F, hop, B, T = 65, 128, 1, 21
    H = R.gpu_H(B, T, F, 21)
    for lpf in range(4):
        r = fz.noise_forward_case(H, hop, mode=(lpf + 1) << 8, against_d=False, **draw(B, T, hop, lpf))
        check(r, f"WAVE+C{lpf}", label="forced")


# ---- D: one frame per workgroup ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,hop,B,T", [(9, 1, 2, 4), (5, 3, 2, 4), (33, 7, 3, 2), (65, 12, 2, 3), (33, 100, 3, 2), (129, 441, 2, 2),
                                       (1025, 2048, 1, 2), (129, 8192, 1, 2)])      # the last: more than 64 KiB of LDS
def test_frame_form(F, hop, B, T):
    natural = fz.noise_fwd_form(B, T, F, hop)
    assert natural == "D" or (F, hop) == (1025, 2048)         # (a tile of 8 frames fits there: mode 1 asks for the frame kernel)
    H = R.gpu_H(B, T, F, F * 10 + hop)
    r = fz.noise_forward_case(H, hop, mode=0 if natural == "D" else 1, **draw(B, T, hop, F + hop))
    check(r, "D")


# ---- pointer facts: views 4 bytes into their storage ---------------------------------------------------------------------------
@pytest.mark.parametrize("F,hop,B,T,which,form", [(65, 128, 1, 33, "y", "D"), (65, 128, 1, 33, "uniform", "C1"), (65, 128, 1, 33, "Hmag", "C1"),
                                                  (195, 512, 2, 9, "y", "D"), (195, 512, 2, 9, "uniform", "C3"), (195, 512, 2, 9, "Hmag", "FFT")])
def test_misaligned_pointers(F, hop, B, T, which, form):
    H = R.gpu_H(B, T, F, F + len(which))
    kw = draw(B, T, hop, 0, "injected") if which == "uniform" else draw(B, T, hop, len(which))
    r = fz.noise_forward_case(H, hop, misalign=(which,), **kw)
    check(r, form, label=f"misaligned {which}")


# ---- accumulate: the output's earlier contents stay, to the rounding of one fp32 sum -------------------------------------------
@pytest.mark.parametrize("F,hop,B,T,mode,form", [(257, 512, 3, 7, 0, "FFT"), (195, 512, 1, 4097, 0, "FFT+IR"), (65, 128, 2, 40, 0, "WAVE"),
                                                 (65, 128, 1, 21, 0, "WAVE+C1"), (33, 40, 1, 100, 0, "C0"), (129, 256, 1, 17, 0, "C2"),
                                                 (33, 100, 3, 8, 0, "D")])
def test_accumulate(F, hop, B, T, mode, form):
    rng = np.random.default_rng(F + hop + T)
    base = (rng.standard_normal((B, T * hop)) * 10.0 ** rng.uniform(-2, 2, size=(B, 1))).astype(np.float32)
    H = R.gpu_H(B, T, F, F + 5)
    r = fz.noise_forward_case(H, hop, mode=mode, accumulate=base, against_d=T < 1000, **draw(B, T, hop, F + 1))
    check(r, form, label="accumulate")


# ---- non-finite magnitudes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,hop,B,T,mode,form", [(257, 512, 3, 7, 0, "FFT"), (195, 512, 3, 7, 0, "FFT"), (129, 256, 3, 7, 4, "FFT"),
                                                 (195, 512, 1, 4097, 0, "FFT+IR"), (65, 128, 2, 40, 0, "WAVE"), (65, 128, 1, 29, 0, "WAVE+C1"),
                                                 (9, 16, 1, 67, 0, "C0"), (129, 256, 1, 17, 0, "C2"), (257, 512, 3, 5, 2, "C3"),
                                                 (33, 100, 3, 8, 0, "D"), (65, 7, 2, 9, 0, "D")])
def test_non_finite_magnitudes_reach_their_own_frame(F, hop, B, T, mode, form):
    """A NaN at one band of frame 4 and +Inf at one band of frame 9: every sample of those two frames is non-finite (each z[n] sums
    every band, and the tap at lag 0 enters every sample), every other frame meets the tolerances.

    What each form does, read from the sources.  The direct kernels (noise_frame_kernel, noise_batched_kernel) and the wavefront form
    keep one accumulator per frame: nothing crosses frames.  The Fft forms (ddsp_noise_fft.hip) put frames 2p and 2p + 1 into the
    real and imaginary parts of one complex sequence.  The equaliser (ddsp_wave_fft.h: frame_scale) takes max |H| with fmaxf, which
    drops a NaN lane -- the scale of a NaN frame is that of its other bands -- and lets an infinite one win, for which frame_scale_of
    takes e = 0: both scales stay finite powers of two, so the partner's own scaling is never spoiled.  But the packed kernel spectrum
    k_a + i k_b goes through complex butterflies and twiddle products (re = ac - bd, im = ad + bc) that mix the two parts, and the
    Hermitian split reads bins g and N - g of both: a non-finite k_a makes every bin of the pair's product non-finite, hence y_b too.
    So there the partner f ^ 1 comes out ENTIRELY non-finite (partners_lost counts it) -- allowed; finite and wrong is not, and a
    partly finite partner fails nonfinite_ok.  With the product (ddsp_noise_ir.hip) every frame is one row of the A operand and one
    row of the result: split3 of a NaN / Inf spoils that row's three bf16 terms only, and the max-|H| column is per row, by fmaxf
    as above; the FFT stage that follows pairs the rows as before.  The frame itself is non-finite in every form: Inf times the
    table's exact zeros (cospif at a quarter turn) gives NaN, which is as non-finite."""
    H = R.gpu_H(B, T, F, F * 3 + hop).reshape(B * T, F)
    if not H[5].any():
        H[5] = H[6]
    H[4, F // 3] = np.nan                                     # frame 4: partner 5 in the paired forms
    H[9, 1] = np.inf                                          # frame 9: partner 8
    H = H.reshape(B, T, F)
    r = fz.noise_forward_case(H, hop, mode=mode, against_d=T < 1000, **draw(B, T, hop, F))
    check(r, form, label="non-finite", zero=False, bad=2)
    if not r["direct"]:
        print(f"\n{form} F {F} hop {hop}: partners lost {r['partners_lost']} of 2")
    else:
        assert r["partners_lost"] == 0
