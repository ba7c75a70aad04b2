"""GPU tests of the chunked oscillator's code AROUND the per-sample chains (csrc/ddsp_osc_chunk.hip).  The totals pass computes
increments for root slots only, puts a row's stores under one ownership predicate and walks four samples per iteration; the
synth walks are the ones test_gpu_chunked.py covers and are walked here on the same inputs, so that a change of the rows they
load shows in the audio.

Every case forces the chunked form (ddsp_osc_set_path(2)) and compares EVERY sample with the CPU oracle at the suite's 1e-5 and
with the frame kernels (ddsp_osc_set_path(1)) at the 2e-6 that test_gpu_chunked.py holds between the two forms; two calls on
the same inputs must agree bit for bit.  The output buffer is filled with NaN before every call.

Chunk lengths are forced with DDSP_OSC_CHUNK_LEN (a test hook).  The library takes a forced length only from one hop upwards
(the chunk totals live where the frame form keeps one entry per frame, so a row has at most as many chunks as frames); below
that the case `library_choice` runs the length the library picks.  Pieces of exactly 32 samples -- one flush -- and chunk starts
32 and 96 samples into a segment come from the boundaries of the lengths 160 and 352 at hop 128 (160, 480; 352).

`both_walks` puts top-harmonic increments on both sides of the quotient reuse's bound in one launch; which walk a wavefront took
cannot be read back by a caller, so the tests hold the audio, not the choice.
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


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


@pytest.fixture
def lib():
    L = ddsp._lib.lib()
    assert L.ddsp_test_hooks_enabled() == 1, "DDSP_TEST_HOOKS=1 must be set before the library is loaded (tests/conftest.py)"
    yield L
    ddsp._lib.check(L.ddsp_osc_set_tiling(0), "ddsp_osc_set_tiling")
    ddsp._lib.check(L.ddsp_osc_set_path(0), "ddsp_osc_set_path")


def run(f0, c, a, hop, sr):
    """Forward through the C ABI into a buffer of this test's own that holds NaN: a path that writes nothing cannot pass."""
    B, T, H = c.shape
    L = ddsp._lib.lib()
    y = torch.full((B, T * hop), float("nan"), device="cuda")
    scratch = torch.empty(L.ddsp_osc_scratch_bytes(B, T, H), device="cuda", dtype=torch.uint8)
    torch.cuda.synchronize()
    rc = L.ddsp_osc_forward_ex(f0.data_ptr(), c.data_ptr(), a.data_ptr(), y.data_ptr(), scratch.data_ptr(), None, None, None,
                               B, T, H, hop, sr, ctypes.c_uint(0), None)
    ddsp._lib.check(rc, "ddsp_osc_forward_ex")
    torch.cuda.synchronize()
    return y


_REFS = {}


def references(lib, key, K, f0, c, a, hop, sr):
    """(oracle, frame kernels) of one input, computed once and shared by the chunk lengths that walk it."""
    if key not in _REFS:
        B, T, H = c.shape
        ddsp._lib.check(lib.ddsp_osc_set_tiling(K), "ddsp_osc_set_tiling")
        ddsp._lib.check(lib.ddsp_osc_set_path(1), "ddsp_osc_set_path")
        assert ddsp._lib.osc_plan(B, T, H, hop, sr)["chunked"] == 0
        y_frame = run(dev(f0), dev(c), dev(a), hop, sr).cpu().numpy()
        ref = oracle.osc_forward(f0, c, a, hop, sr)
        ref.setflags(write=False)
        y_frame.setflags(write=False)
        _REFS[key] = (ref, y_frame)
    return _REFS[key]


def check(lib, monkeypatch, key, K, G, f0, c, a, hop, sr, chunk_len):
    B, T, H = c.shape
    ref, y_frame = references(lib, key, K, f0, c, a, hop, sr)
    if chunk_len is None:
        monkeypatch.delenv("DDSP_OSC_CHUNK_LEN", raising=False)
    else:
        assert chunk_len >= hop and chunk_len % 32 == 0
        monkeypatch.setenv("DDSP_OSC_CHUNK_LEN", str(chunk_len))
    ddsp._lib.check(lib.ddsp_osc_set_tiling(K), "ddsp_osc_set_tiling")
    ddsp._lib.check(lib.ddsp_osc_set_path(2), "ddsp_osc_set_path")
    plan = ddsp._lib.osc_plan(B, T, H, hop, sr)
    assert plan["chunked"] == 1 and plan["harmonics_per_lane"] == K and plan["lanes_per_row"] == G, plan
    if chunk_len is not None:
        assert plan["chunk_samples"] == chunk_len, plan
    x = (dev(f0), dev(c), dev(a))
    y1 = run(*x, hop, sr)
    y2 = run(*x, hop, sr)
    assert torch.equal(y1, y2)
    y = y1.cpu().numpy()
    assert np.isfinite(y).all()
    e_ref, e_frame = float(np.max(np.abs(y - ref))), float(np.max(np.abs(y - y_frame)))
    print(f"{key} chunks of {plan['chunk_samples']}: max |chunked - oracle| = {e_ref:.3e}, max |chunked - frame kernels| = {e_frame:.3e}")
    assert e_ref <= TOL_Y
    assert e_frame <= TOL_FORMS


def all_live(B, T, H, sr, seed):
    ctl = syn.make_controls(syn.SynthShape("t", B, sr, 128, T, H, 65), seed, "all_live")
    return ctl["f0"], ctl["c"], ctl["a"]


def both_walks(B, T, H, sr, seed):
    """All-live rows (every increment below the reuse bound: the pair walk) in which some frames of some rows jump to 300 .. 400 Hz:
    the frame before still has every harmonic audible, so the chunk walks all slots, and the top increments are beyond
    the bound, so that wavefront takes the walk that computes every quotient.  Both kinds of wavefront in one launch."""
    f0, c, a = all_live(B, T, H, sr, seed)
    top = 2.0 * np.pi * H * f0 / sr
    assert float(top.max()) < REUSE_MAX_INC
    rng = np.random.default_rng(seed + 1)
    for b in range(1, B, 3):
        t = int(rng.integers(1, T))
        f0[b, t:, 0] = rng.uniform(300.0, 400.0, T - t).astype(np.float32)
    top = 2.0 * np.pi * H * f0 / sr
    assert float(top.min()) < REUSE_MAX_INC < float(top.max())
    assert bool((top.max(axis=(1, 2)) < REUSE_MAX_INC).any())      # rows that stay on the pair walk throughout
    return f0, c, a


# ---- pieces of 32 samples and longer, chunk starts 32 and 96 samples into a segment: one full wavefront of 8 rows, one with a single row -------------------------------------
LIBRARY_CHOICE = pytest.param(None, id="library_choice")


@pytest.mark.parametrize("hop,chunk_len", [(128, None), (128, 160), (128, 352), (64, None), (64, 96), (64, 160), (64, 352)],
                         ids=lambda v: "library_choice" if v is None else str(v))
def test_both_walks_every_piece_length(lib, monkeypatch, hop, chunk_len):
    B, T, H, sr = 9, 6, 100, 16000
    f0, c, a = both_walks(B, T, H, sr, 600 + hop)
    check(lib, monkeypatch, f"pair_hop{hop}", 13, 8, f0, c, a, hop, sr, chunk_len)


# ---- lane counts --------------------------------------------------------------------------------------------------
LANES = [
    # B, H, K, lanes per row
    (17, 60, 15, 4),      # 15 x 4: 16 rows per wavefront, 8 + 7 slots
    (5, 200, 13, 16),     # 13 x 16: 4 rows per wavefront
    (9, 50, 13, 4),       # the all-roots fallback (the 7 + 6 shape does not pack 50 harmonics on 4 lanes)
]


@pytest.mark.parametrize("chunk_len", [LIBRARY_CHOICE, 160])
@pytest.mark.parametrize("B,H,K,G", LANES)
def test_lane_counts(lib, monkeypatch, B, H, K, G, chunk_len):
    T, hop, sr = 6, 128, 16000
    f0, c, a = both_walks(B, T, H, sr, 700 + H)
    check(lib, monkeypatch, f"lanes_h{H}", K, G, f0, c, a, hop, sr, chunk_len)


# ---- who stores a row: clips of two and three frames, chunk boundaries on and just behind a segment's start ---------------
# hop 128: segments start at 64 + 128 s.  192 puts a boundary on a start; 224 one 32-block behind one (192 + 32) and, in the
# three-frame clip, none further; 128 cuts every segment in the middle; 160 ends 32 samples before a start.
@pytest.mark.parametrize("chunk_len", [128, 160, 192, 224])
@pytest.mark.parametrize("B,T", [(9, 2), (9, 3), (1, 2), (1, 3), (1, 6)])
def test_row_ownership(lib, monkeypatch, B, T, chunk_len):
    H, hop, sr = 100, 128, 16000
    f0, c, a = all_live(B, T, H, sr, 800 + 10 * B + T)
    check(lib, monkeypatch, f"own_b{B}_t{T}", 13, 8, f0, c, a, hop, sr, chunk_len)


@pytest.mark.parametrize("chunk_len", [64, 96, 160])     # hop 64: segments start at 32 + 64 s; 96 = a start, 160 = a start, 64 = mid-segment
def test_row_ownership_smallest_hop(lib, monkeypatch, chunk_len):
    B, T, H, hop, sr = 5, 3, 100, 64, 16000
    f0, c, a = all_live(B, T, H, sr, 877)
    check(lib, monkeypatch, "own_hop64", 13, 8, f0, c, a, hop, sr, chunk_len)


# ---- the short walks (silent harmonics) are not touched and stay as they were ------------------------------------------
def test_musical_f0_reaches_three_silent_classes(lib, monkeypatch):
    B, T, H, hop, sr = 40, 6, 100, 128, 16000
    ctl = syn.make_controls(syn.SynthShape("t", B, sr, hop, T, H, 65), 901, "musical")
    f0, c, a = ctl["f0"], ctl["c"], ctl["a"]
    # highest audible harmonic of a row anywhere in the clip; the class limits of 100 harmonics on 8 lanes are 89, 60, 26, 12.
    # A wavefront takes the class of the highest of its 8 rows (rows are ordered by class): every 8th of the sorted tops.
    tops = np.sort(np.minimum(np.floor(0.5 * sr / f0[:, :, 0].min(axis=1)), H))[::-1]
    classes = {int(np.searchsorted([12, 26, 60, 89], t)) for t in tops[::8]}
    assert len(classes) >= 3, (tops, classes)
    for chunk_len in (160, 352):
        check(lib, monkeypatch, "musical", 13, 8, f0, c, a, hop, sr, chunk_len)
