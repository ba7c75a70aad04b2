"""GPU tests of the chunked oscillator's DERIVED slots (csrc/ddsp_osc_chunk.hip, csrc/ddsp_osc_plan.h): a lane walks the
increment / fp64 accumulate chain only for its root slots and takes the phase of harmonic 2^t * r as 2^t times the rounded phase
of harmonic r.  Each case runs the production mapping and the all-roots mapping (DDSP_OSC_CHUNK_ALL_ROOTS=1, a test hook) and
holds the first against the CPU oracle at the suite's 1e-5 and against the second at 2e-6 -- the bound
test_gpu_chunked.py::test_chunked_vs_oracle_and_frame_kernels holds between two summation orders of the same terms.

H = 1, 2, 3 cannot reach the chunked form at all (it needs at least 4 lanes per row, i.e. more than 2 * 4 harmonics); they run
through whatever the library picks, so that the planner's fallback is at least never in the way.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ddsp_pytorch_amd as ddsp  # noqa: E402
from ddsp_pytorch_amd import synthetic as syn  # noqa: E402
from oracle import oracle  # noqa: E402

TOL_Y = 1e-5
TOL_ARMS = 2e-6


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
    y, _, _ = ddsp.osc_forward(dev(f0), dev(c), dev(a), hop, sr)
    torch.cuda.synchronize()
    return y.cpu().numpy()


def force_chunked(L, K, B, T, H, hop, sr):
    ddsp._lib.check(L.ddsp_osc_set_tiling(K), "ddsp_osc_set_tiling")
    ddsp._lib.check(L.ddsp_osc_set_path(2), "ddsp_osc_set_path")
    plan = ddsp._lib.osc_plan(B, T, H, hop, sr)
    assert plan["chunked"] == 1 and plan["harmonics_per_lane"] == K, plan
    return plan


def both_arms(monkeypatch, f0, c, a, hop, sr):
    monkeypatch.delenv("DDSP_OSC_CHUNK_ALL_ROOTS", raising=False)
    y = run(f0, c, a, hop, sr)
    monkeypatch.setenv("DDSP_OSC_CHUNK_ALL_ROOTS", "1")
    y_roots = run(f0, c, a, hop, sr)
    monkeypatch.delenv("DDSP_OSC_CHUNK_ALL_ROOTS")
    return y, y_roots


def report(tag, y, y_roots, ref, ok=None):
    ok = np.ones(ref.shape, bool) if ok is None else ok
    e_ref, e_arm = float(np.max(np.abs(y[ok] - ref[ok]))), float(np.max(np.abs(y[ok] - y_roots[ok])))
    print(f"{tag}: max |derived - oracle| = {e_ref:.3e}, max |derived - all roots| = {e_arm:.3e}")
    return e_ref, e_arm


def controls(B, T, H, sr, kind, seed):
    ctl = syn.make_controls(syn.SynthShape("t", B, sr, 128, T, H, 65), seed, kind)
    return ctl["f0"], ctl["c"], ctl["a"]


# (B, T, H, hop, sr, K, lanes per row, derived slots expected)
SHAPES = [
    (9, 37, 100, 128, 16000, 13, 8, True),
    (5, 23, 200, 512, 48000, 13, 16, True),
    (3, 19, 60, 64, 16000, 15, 4, True),
    (2, 11, 180, 512, 44100, 12, 16, True),
    (17, 7, 50, 256, 16000, 13, 4, False),      # the 7 + 6 shape does not pack 50 harmonics on 4 lanes: all roots
    (3, 5, 64, 4096, 16000, 16, 4, True),
    (6, 21, 100, 128, 16000, 25, 4, True),
]


@pytest.mark.parametrize("kind", ["all_live", "musical"])
@pytest.mark.parametrize("B,T,H,hop,sr,K,G,derived", SHAPES)
def test_derived_slots_vs_oracle_and_all_roots(lib, monkeypatch, B, T, H, hop, sr, K, G, derived, kind):
    f0, c, a = controls(B, T, H, sr, kind, 1234 + H + T)
    plan = force_chunked(lib, K, B, T, H, hop, sr)
    assert plan["lanes_per_row"] == G
    y, y_roots = both_arms(monkeypatch, f0, c, a, hop, sr)
    ref = oracle.osc_forward(f0, c, a, hop, sr)
    e_ref, e_arm = report(f"H={H} K={K} G={G} {kind}", y, y_roots, ref)
    assert np.isfinite(y).all()
    assert e_ref <= TOL_Y and float(np.max(np.abs(y_roots - ref))) <= TOL_Y
    assert e_arm <= TOL_ARMS
    # the hook selects another mapping (another summation order), or none where the planner falls back
    assert bool(np.any(y != y_roots)) == derived


@pytest.mark.parametrize("H", [1, 2, 3])
def test_fewest_harmonics(lib, monkeypatch, H):
    B, T, hop, sr = 8, 12, 128, 16000
    f0, c, a = controls(B, T, H, sr, "all_live", 50 + H)
    y, y_roots = both_arms(monkeypatch, f0, c, a, hop, sr)
    ref = oracle.osc_forward(f0, c, a, hop, sr)
    e_ref, e_arm = report(f"H={H}", y, y_roots, ref)
    assert e_ref <= TOL_Y and e_arm <= TOL_ARMS


def test_all_five_silent_harmonic_classes(lib, monkeypatch):
    """Rows whose highest audible harmonic is 100, 80, 50, 20, 8, 2 or 1 (constant f0, Nyquist 8 kHz): eight of each, so that
    after the per-chunk ordering whole wavefronts stop at each of the five walk lengths (class limits at 100 harmonics on
    8 lanes: 89, 60, 26, 12).  Highest audible = 2 is a derived slot above silent roots; = 1 leaves only a root audible."""
    B, T, H, hop, sr = 56, 30, 100, 128, 16000
    tops = [100, 80, 50, 20, 8, 2, 1]
    rng = np.random.default_rng(31)
    f0 = np.empty((B, T, 1), np.float32)
    for b in range(B):
        top = tops[b % len(tops)]
        f0[b] = np.float32(8000.0 / (top + 0.5))
    c = rng.uniform(0.1, 1.0, (B, T, H)).astype(np.float32)
    a = rng.uniform(0.1, 1.0, (B, T, 1)).astype(np.float32)
    force_chunked(lib, 13, B, T, H, hop, sr)
    y, y_roots = both_arms(monkeypatch, f0, c, a, hop, sr)
    ref = oracle.osc_forward(f0, c, a, hop, sr)
    for i, top in enumerate(tops):
        rows = np.arange(i, B, len(tops))
        e_ref, e_arm = report(f"highest audible {top}", y[rows], y_roots[rows], ref[rows])
        assert e_ref <= TOL_Y and e_arm <= TOL_ARMS
    # a row that changes class along the clip: the audible top falls from 100 to 3 and rises again
    f0v = f0.copy()
    f0v[:, :, 0] = np.concatenate([np.linspace(70.0, 2500.0, T // 2), np.linspace(2500.0, 70.0, T - T // 2)]).astype(np.float32)
    y, y_roots = both_arms(monkeypatch, f0v, c, a, hop, sr)
    e_ref, e_arm = report("gliding top", y, y_roots, oracle.osc_forward(f0v, c, a, hop, sr))
    assert e_ref <= TOL_Y and e_arm <= TOL_ARMS


def test_derived_slot_trips_the_reuse_and_range_checks(lib, monkeypatch):
    """Harmonic 100 is a derived slot (root 25 feeds 50 and 100).  Its increment crosses the quotient reuse's bound (4.8 rad per sample)
    and its phase the fast modulo's exact range (1e7 rad) while harmonic 25's do neither: the checks must look at 2^t times the
    root's values.  Row 0: only harmonic 100 is above 4.8 (99 is not); rows 1, 2: 100 well above, 25 below; row 3 (8 kHz, hop
    512, long clip) is in the second call: harmonic 100 reaches 3.5e7 rad, harmonic 25 stays below 1e7."""
    rng = np.random.default_rng(41)
    B, T, H, hop, sr = 8, 40, 100, 128, 16000
    f0 = np.full((B, T, 1), 100.0, np.float32)
    f0[0] = 122.8       # 100 * f0 * 2pi / sr = 4.822, 99 * ... = 4.774
    f0[1] = 300.0       # harmonic 100: 11.8, harmonic 25: 2.95
    f0[2] = 480.0       # harmonic 100: 18.8, harmonic 25: 4.71
    c = rng.uniform(0.1, 1.0, (B, T, H)).astype(np.float32)
    a = rng.uniform(0.1, 1.0, (B, T, 1)).astype(np.float32)
    force_chunked(lib, 13, B, T, H, hop, sr)
    y, y_roots = both_arms(monkeypatch, f0, c, a, hop, sr)
    e_ref, e_arm = report("reuse bound", y, y_roots, oracle.osc_forward(f0, c, a, hop, sr))
    assert e_ref <= TOL_Y and e_arm <= TOL_ARMS

    B, T, H, hop, sr = 4, 300, 100, 512, 8000
    f0 = rng.uniform(30.0, 39.0, (B, T, 1)).astype(np.float32)
    f0[3] = 2900.0      # harmonic 1 audible; harmonic 100: 227.8 rad per sample -> 3.5e7 rad, harmonic 25 -> 8.7e6 rad
    c = rng.uniform(0.1, 1.0, (B, T, H)).astype(np.float32)
    a = rng.uniform(0.1, 1.0, (B, T, 1)).astype(np.float32)
    force_chunked(lib, 13, B, T, H, hop, sr)
    y, y_roots = both_arms(monkeypatch, f0, c, a, hop, sr)
    e_ref, e_arm = report("phase range", y, y_roots, oracle.osc_forward(f0, c, a, hop, sr))
    assert e_ref <= TOL_Y and e_arm <= TOL_ARMS


def test_tiny_increments(lib, monkeypatch):
    """f0 = 1e-30 (and smaller, down to increments that are subnormal in fp32, where 2 * fl(x) and fl(2 * x) may part): the phases
    involved are below 1e-25 rad, so whatever the doubling loses is far below the tolerance; no separate walk is needed."""
    rng = np.random.default_rng(43)
    B, T, H, hop, sr = 8, 20, 100, 128, 16000
    f0, c, a = controls(B, T, H, sr, "all_live", 9)
    f0[1] = 1e-30
    f0[2, 5:9] = 1e-30
    f0[3] = 1e-36          # increments ~4e-40: subnormal
    f0[4, ::2] = 3e-38
    force_chunked(lib, 13, B, T, H, hop, sr)
    y, y_roots = both_arms(monkeypatch, f0, c, a, hop, sr)
    e_ref, e_arm = report("tiny f0", y, y_roots, oracle.osc_forward(f0, c, a, hop, sr))
    assert np.isfinite(y).all()
    assert e_ref <= TOL_Y and e_arm <= TOL_ARMS


def test_negative_and_nan_rows_are_repaired(lib, monkeypatch):
    B, T, H, hop, sr = 8, 24, 100, 128, 16000
    f0, c, a = controls(B, T, H, sr, "musical", 12)
    f0[2, 5:9, 0] = -220.0
    f0[5, 7, 0] = np.nan
    force_chunked(lib, 13, B, T, H, hop, sr)
    y, y_roots = both_arms(monkeypatch, f0, c, a, hop, sr)
    ref = oracle.osc_forward(f0, c, a, hop, sr)
    ok = np.isfinite(ref)
    assert np.array_equal(np.isfinite(y), ok) and np.array_equal(np.isfinite(y_roots), ok)
    e_ref, e_arm = report("negative / NaN f0", y, y_roots, ref, ok)
    assert e_ref <= TOL_Y and e_arm <= TOL_ARMS


def test_derived_slots_are_deterministic(lib, monkeypatch):
    monkeypatch.delenv("DDSP_OSC_CHUNK_ALL_ROOTS", raising=False)
    B, T, H, hop, sr = 24, 60, 100, 128, 16000
    f0, c, a = controls(B, T, H, sr, "musical", 8)
    force_chunked(lib, 13, B, T, H, hop, sr)
    y = run(f0, c, a, hop, sr)
    assert np.array_equal(y, run(f0, c, a, hop, sr))
