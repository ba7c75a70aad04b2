"""GPU tests of the chunked oscillator's derived slots with COMPILE-TIME factors (csrc/ddsp_osc_chunk.hip: walk_synth).

A derived slot's phase is 2^t times its root's, and t is a property of the slot (csrc/ddsp_osc_plan.h: derived_shift), so the fast
walk never forms that phase: it runs the modulo on the root's phase with constants that carry 2^t.  The exact walk multiplies by
the compile-time 2^t, and the two range tests (quotient reuse, fast modulo) scale their bounds by it and skip padded derived
slots through a per-lane mask.  Every shape the library ships with derived slots is here, three of them with padded derived
slots (4 at 100 x 13 x 8, 7 at 200 x 13 x 16, 12 at 180 x 12 x 16).

Conventions of test_gpu_osc_chunk_trim.py: the chunked form is forced (ddsp_osc_set_path(2)), the output buffer holds NaN before
every call, two calls on the same inputs agree bit for bit, every sample is held against the CPU oracle at the suite's 1e-5 and
against the frame kernels (ddsp_osc_set_path(1)) at the 2e-6 that test_gpu_chunked.py holds between the two forms -- and at the
same 2e-6 against the all-roots mapping (DDSP_OSC_CHUNK_ALL_ROOTS=1, a test hook), which has no derived slot at all.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ddsp_pytorch_amd as ddsp  # noqa: E402
from ddsp_pytorch_amd import synthetic as syn  # noqa: E402
from oracle import oracle  # noqa: E402

TOL_Y = 1e-5
TOL_FORMS = 2e-6
REUSE_MAX_INC = 4.8     # kReuseMaxInc: a wavefront reuses the modulo's quotient while every increment of its rows is below
T, SR = 6, 16000

# B, H, K, lanes per row: every shipped shape with derived slots.  9 rows at 8 per wavefront, 17 at 16, 5 at 4: a full wavefront and
# a one-row one (9 rows at 16 or at 4 per wavefront: a partly filled one, two full ones and a one-row one)
SHAPES = [
    (9, 100, 13, 8),
    (5, 200, 13, 16),
    (17, 60, 15, 4),
    (9, 64, 16, 4),
    (9, 180, 12, 16),
]
SHAPE_IDS = [f"{H}x{K}x{G}" for _, H, K, G in SHAPES]


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


@pytest.fixture
def lib(monkeypatch):
    L = ddsp._lib.lib()
    assert L.ddsp_test_hooks_enabled() == 1, "DDSP_TEST_HOOKS=1 must be set before the library is loaded (tests/conftest.py)"
    monkeypatch.delenv("DDSP_OSC_CHUNK_LEN", raising=False)
    monkeypatch.delenv("DDSP_OSC_CHUNK_ALL_ROOTS", raising=False)
    yield L
    ddsp._lib.check(L.ddsp_osc_set_tiling(0), "ddsp_osc_set_tiling")
    ddsp._lib.check(L.ddsp_osc_set_path(0), "ddsp_osc_set_path")


def run(f0, c, a, hop, sr):
    """Forward through the C ABI into a buffer of this test's own that holds NaN: a path that writes nothing cannot pass."""
    B, T_, H = c.shape
    L = ddsp._lib.lib()
    y = torch.full((B, T_ * hop), float("nan"), device="cuda")
    scratch = torch.empty(L.ddsp_osc_scratch_bytes(B, T_, H), device="cuda", dtype=torch.uint8)
    torch.cuda.synchronize()
    rc = L.ddsp_osc_forward_ex(f0.data_ptr(), c.data_ptr(), a.data_ptr(), y.data_ptr(), scratch.data_ptr(), None, None, None,
                               B, T_, H, hop, sr, ctypes.c_uint(0), None)
    ddsp._lib.check(rc, "ddsp_osc_forward_ex")
    torch.cuda.synchronize()
    return y


def check(lib, monkeypatch, tag, K, G, f0, c, a, hop, nonfinite=False):
    B, T_, H = c.shape
    x = (dev(f0), dev(c), dev(a))
    ref = oracle.osc_forward(f0, c, a, hop, SR)
    ddsp._lib.check(lib.ddsp_osc_set_tiling(K), "ddsp_osc_set_tiling")
    ddsp._lib.check(lib.ddsp_osc_set_path(1), "ddsp_osc_set_path")
    assert ddsp._lib.osc_plan(B, T_, H, hop, SR)["chunked"] == 0
    y_frame = run(*x, hop, SR).cpu().numpy()
    ddsp._lib.check(lib.ddsp_osc_set_path(2), "ddsp_osc_set_path")
    plan = ddsp._lib.osc_plan(B, T_, H, hop, SR)
    assert plan["chunked"] == 1 and plan["harmonics_per_lane"] == K and plan["lanes_per_row"] == G, plan
    monkeypatch.setenv("DDSP_OSC_CHUNK_ALL_ROOTS", "1")
    y_roots = run(*x, hop, SR).cpu().numpy()
    monkeypatch.delenv("DDSP_OSC_CHUNK_ALL_ROOTS")
    y1 = run(*x, hop, SR)
    y2 = run(*x, hop, SR)
    assert torch.equal(y1.view(torch.int32), y2.view(torch.int32))      # bit for bit, NaN included
    y = y1.cpu().numpy()
    ok = np.isfinite(ref)
    if nonfinite:
        assert not ok.all()
        for other in (y, y_roots):
            assert np.array_equal(np.isfinite(other), ok)
    else:
        assert ok.all() and np.isfinite(y).all()
    assert bool(np.any(y[ok] != y_roots[ok]))        # the hook did select another mapping: the comparison arm has no derived slot
    e_ref, e_frame, e_roots = (float(np.max(np.abs(y[ok] - o[ok]))) for o in (ref, y_frame, y_roots))
    print(f"{tag} hop {hop} chunks of {plan['chunk_samples']}: max |chunked - oracle| = {e_ref:.3e}, "
          f"|chunked - frame kernels| = {e_frame:.3e}, |chunked - all roots| = {e_roots:.3e}")
    assert e_ref <= TOL_Y
    assert e_frame <= TOL_FORMS
    assert e_roots <= TOL_FORMS


def all_live(B, H, seed):
    ctl = syn.make_controls(syn.SynthShape("t", B, SR, 128, T, H, 65), seed, "all_live")
    return ctl["f0"], ctl["c"], ctl["a"]


def both_walks(B, H, seed):
    """test_gpu_osc_chunk_trim.py's construction: all-live rows (every increment below the reuse bound) in which some frames of some
    rows jump to 300 .. 400 Hz while the frame before still has every harmonic audible, so the chunk walks all slots and that
    wavefront computes every quotient -- both quotient modes in one launch.  At 100 harmonics row 0 moves to 122.8 Hz instead:
    harmonic 100 = 4 x 25, a derived slot, is then the ONLY one beyond the bound (4.822; harmonic 99: 4.774, harmonic 25: 1.206),
    so the walk is chosen by the derived slots' test alone."""
    f0, c, a = all_live(B, H, seed)
    top = 2.0 * np.pi * H * f0 / SR
    assert float(top.max()) < REUSE_MAX_INC
    rng = np.random.default_rng(seed + 1)
    for b in range(1, B, 3):
        t = int(rng.integers(1, T))
        f0[b, t:, 0] = rng.uniform(300.0, 400.0, T - t).astype(np.float32)
    if H == 100:
        f0[0, 3:, 0] = 122.8
        inc = 2.0 * np.pi * np.float64(np.float32(122.8)) / SR
        assert 99 * inc < REUSE_MAX_INC < 100 * inc
    top = 2.0 * np.pi * H * f0 / SR
    assert float(top.min()) < REUSE_MAX_INC < float(top.max())
    assert bool((top.max(axis=(1, 2)) < REUSE_MAX_INC).any())      # rows that stay on the pair walk throughout
    return f0, c, a


def musical(B, H, seed):
    ctl = syn.make_controls(syn.SynthShape("t", B, SR, 128, T, H, 65), seed, "musical")
    return ctl["f0"], ctl["c"], ctl["a"]


INPUTS = {"all_live": all_live, "both_walks": both_walks, "musical": musical}


@pytest.mark.parametrize("kind", list(INPUTS))
@pytest.mark.parametrize("hop", [128, 64])
@pytest.mark.parametrize("B,H,K,G", SHAPES, ids=SHAPE_IDS)
def test_compile_time_factors_vs_oracle_frames_and_all_roots(lib, monkeypatch, B, H, K, G, hop, kind):
    f0, c, a = INPUTS[kind](B, H, 1000 + H + K + hop)
    check(lib, monkeypatch, f"{H}x{K}x{G} {kind}", K, G, f0, c, a, hop)


@pytest.mark.parametrize("hop", [128, 64])
def test_musical_f0_reaches_three_silent_classes(lib, monkeypatch, hop):
    B, H = 40, 100
    f0, c, a = musical(B, H, 901)
    # highest audible harmonic of a row anywhere in the clip; the class limits of 100 harmonics on 8 lanes are 89, 60, 26, 12.
    # A wavefront takes the class of the highest of its 8 rows (rows are ordered by class): every 8th of the sorted tops.
    tops = np.sort(np.minimum(np.floor(0.5 * SR / f0[:, :, 0].min(axis=1)), H))[::-1]
    classes = {int(np.searchsorted([12, 26, 60, 89], t)) for t in tops[::8]}
    assert len(classes) >= 3, (tops, classes)
    check(lib, monkeypatch, "musical classes", 13, 8, f0, c, a, hop)


@pytest.mark.parametrize("B,H,K,G", SHAPES, ids=SHAPE_IDS)
def test_declined_chunks_take_the_exact_walk(lib, monkeypatch, B, H, K, G):
    """A negative f0 stretch and a NaN f0 frame: the wavefronts that hold them decline their chunks and walk them again with the
    exact modulo, which multiplies the root's phase by the compile-time 2^t.  Compared wherever the oracle is finite; the
    non-finite samples must be the same ones."""
    f0, c, a = musical(B, H, 77 + H)
    f0[1, 2:4, 0] = -220.0
    f0[3, 4, 0] = np.nan
    check(lib, monkeypatch, f"{H}x{K}x{G} negative / NaN f0", K, G, f0, c, a, 128, nonfinite=True)
