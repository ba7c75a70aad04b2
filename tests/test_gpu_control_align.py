"""The time alignment on the device (csrc/ddsp_align.hip) against tests/control_align_reference.py: the kernel's cost, path and
length are those of `dtw_fp32`, the kernel's arithmetic operation by operation, bit for bit; its positions are the fp64 timeline of
its own path, rounded once.  Then what the alignment is for: a phrase and its slower, transposed second take, through
`align_controls` and `morph_controls`, and `AutoEncoder.morph(..., align=True)`.  Every test prints its observed figure before
it asserts."""
import functools

import numpy as np
import pytest
import torch

import ddsp_pytorch_amd as ddsp
import control_align_reference as ref
from ddsp_pytorch_amd import analysis
from encoder_common import AEConf

pytestmark = pytest.mark.gpu

SR = ref.SAMPLE_RATE


def cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def same_bits(x, y):
    return x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x.view(np.uint32), y.view(np.uint32))


def ulps(x, y):
    return np.abs(x.view(np.int32).astype(np.int64) - y.view(np.int32).astype(np.int64))


def device(xa, xb, **keywords):
    out = ddsp.dtw_align(cuda(xa), cuda(xb), return_path=True, **keywords)
    assert all(v.is_cuda for v in out)
    assert [v.dtype for v in out] == [torch.float32, torch.float32, torch.int32, torch.int32, torch.float32]
    return [v.cpu().numpy() for v in out]


@functools.lru_cache(maxsize=None)
def emulation(case):
    """The inputs of one case and `dtw_fp32` of every row: computed once, shared, not modified."""
    B, T_a, T_b, D, radius, penalty = case
    xa, xb = ref.sequences(B, T_a, T_b, D)
    return xa, xb, [ref.dtw_fp32(xa[b], xb[b], radius, penalty) for b in range(B)]


def check(got, want, T_a, T_b, timing, frames=None):
    """The device's five outputs against the emulation's (path, cost) per row -> the positions' largest distance, in ulps, from
    the fp64 timeline of the device's own path."""
    pos_a, pos_b, path, length, cost = got
    worst = 0
    for b, (want_path, want_cost) in enumerate(want):
        n = int(length[b])
        assert n == len(want_path) and max(T_a, T_b) <= n <= T_a + T_b - 1, b
        assert np.array_equal(path[b, :n], want_path) and (path[b, n:] == -1).all(), b
        assert same_bits(cost[b:b + 1], np.array([want_cost], np.float32)), (b, cost[b], want_cost)
        wa, wb = ref.timeline(path[b, :n].astype(np.int64), T_a, T_b, timing, frames)
        assert pos_a[b].shape == wa.shape
        for pos, line, T in ((pos_a[b], wa, T_a), (pos_b[b], wb, T_b)):
            assert (np.diff(pos) >= 0).all() and pos[0] >= 0 and pos[-1] <= T - 1, b
            worst = max(worst, int(ulps(pos, line.astype(np.float32)).max()))
    return worst


@pytest.mark.parametrize("case", ref.GPU_CASES, ids=str)
def test_kernel_is_the_emulation_bit_for_bit(case):
    B, T_a, T_b, D, radius, penalty = case
    xa, xb, want = emulation(case)
    worst = 0
    for timing, frames in [(t, None) for t in ref.TIMINGS] + [(0.3, 2 * T_a + 3), (0.5, 1)]:
        got = device(xa, xb, radius=radius, penalty=penalty, timing=timing, frames=frames)
        worst = max(worst, check(got, want, T_a, T_b, timing, frames))
        if frames is None and timing == 0.0:
            assert np.array_equal(got[0], np.tile(np.arange(T_a, dtype=np.float32), (B, 1)))      # A's clock, exactly
        if frames is None and timing == 1.0:
            assert np.array_equal(got[1], np.tile(np.arange(T_b, dtype=np.float32), (B, 1)))
    print(f"{case}: cost, path and length are the emulation's; positions within {worst} ulp of the fp64 timeline of the path")
    assert worst <= 1


@pytest.mark.parametrize("T_a,D", ref.WARP_SHAPES)
def test_warped_copies_are_found_exactly(T_a, D):
    xa, xb, w = ref.warped_copy(T_a, D)
    T_b = len(w)
    pos_a, pos_b, path, length, cost = device(xa[None], xb[None], timing=1.0)
    print(f"a copy of {T_a} frames warped onto {T_b}: cost {cost[0]!r}, {int((path[0, :T_b, 0] == w).sum())} of {T_b} path points on w")
    assert int(length[0]) == T_b and np.array_equal(path[0, :T_b], np.stack([w, np.arange(T_b)], 1)) and cost[0] == 0.0
    assert np.array_equal(pos_a[0], w.astype(np.float32)) and np.array_equal(pos_b[0], np.arange(T_b, dtype=np.float32))


def test_ties_follow_the_rule():
    """All features equal, so every cost is 0 and only the order of the comparisons decides."""
    worst = 0
    for T_a, T_b, penalty in ((7, 7, 0.0), (5, 70, 0.0), (70, 5, 0.0), (66, 67, 0.25)):
        xa, xb = np.full((2, T_a, 3), 1.5, np.float32), np.full((2, T_b, 3), 1.5, np.float32)
        want = [ref.dtw_fp32(xa[b], xb[b], None, penalty) for b in range(2)]
        worst = max(worst, check(device(xa, xb, penalty=penalty, timing=0.5), want, T_a, T_b, 0.5))
        assert (np.diff(want[0][0], axis=0)[-(min(T_a, T_b) - 1):] == 1).all()                     # the diagonal wherever it exists
    print(f"ties: the emulation's paths; positions within {worst} ulp")
    assert worst <= 1


def test_hostile_values_stay_inside_the_buffers():
    """NaN, +-inf and 3e38 in both inputs and a row that is all NaN, handed to the entry point itself with a guard zone behind every
    output and behind the workspace: the outputs are the definition's, every index is inside its range, nothing else is written."""
    B, T_a, T_b, D, T_out, GUARD, MARK = 3, 70, 45, 5, 50, 256, -7
    xa, xb = ref.hostile(B, T_a, T_b, D)
    assert np.isnan(xa[-1]).all() and np.isinf(xa).any() and np.isnan(xb).any() and (np.abs(xb[np.isfinite(xb)]) > 1e38).any()
    L = ddsp._lib.lib()
    nbytes = L.ddsp_dtw_workspace_bytes(B, T_a, T_b)
    longest = T_a + T_b - 1
    pos = [torch.full((B * T_out + GUARD,), float(MARK), device="cuda") for _ in range(2)]
    path = torch.full((B * longest * 2 + GUARD,), MARK, dtype=torch.int32, device="cuda")
    length = torch.full((B + GUARD,), MARK, dtype=torch.int32, device="cuda")
    cost = torch.full((B + GUARD,), float(MARK), device="cuda")
    work = torch.full((nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    a, b = cuda(xa), cuda(xb)
    for radius, penalty in ((0, 0.0), (3, 0.01)):
        rc = L.ddsp_dtw_align(a.data_ptr(), b.data_ptr(), pos[0].data_ptr(), pos[1].data_ptr(), path.data_ptr(), length.data_ptr(),
                              cost.data_ptr(), work.data_ptr(), nbytes, B, T_a, T_b, D, T_out, radius, penalty, 0.5,
                              torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        torch.cuda.synchronize()
        assert all(bool((v[-GUARD:] == MARK).all()) for v in (pos[0], pos[1], path, length, cost)) and bool((work[-GUARD:] == 0xA5).all())
        got = [pos[0][:-GUARD].reshape(B, T_out).cpu().numpy(), pos[1][:-GUARD].reshape(B, T_out).cpu().numpy(),
               path[:-GUARD].reshape(B, longest, 2).cpu().numpy(), length[:-GUARD].cpu().numpy(), cost[:-GUARD].cpu().numpy()]
        want = [ref.dtw_fp32(xa[r], xb[r], radius or None, penalty) for r in range(B)]
        worst = check(got, want, T_a, T_b, 0.5, T_out)
        n = got[3]
        inside = all(((got[2][r, :n[r]] >= 0) & (got[2][r, :n[r]] < (T_a, T_b))).all() for r in range(B))
        print(f"hostile values, radius {radius}: costs {got[4]}, lengths {n}; positions within {worst} ulp; every index inside: {inside}")
        assert inside and worst <= 1 and np.isinf(got[4][-1]) and np.isfinite(got[4][0])
        assert (got[0] >= 0).all() and (got[0] <= T_a - 1).all() and (got[1] >= 0).all() and (got[1] <= T_b - 1).all()


def test_deterministic_and_rows_independent():
    case = (3, 5, 40, 2, 1, 0.0)
    xa, xb, _ = emulation(case)
    kw = dict(radius=1, timing=0.5)
    first, again = device(xa, xb, **kw), device(xa, xb, **kw)
    flipped, alone = device(xa[::-1], xb[::-1], **kw), device(xa[1:2], xb[1:2], **kw)
    for k in range(5):
        view = (lambda v: v.view(np.uint32)) if first[k].dtype == np.float32 else (lambda v: v)
        assert np.array_equal(view(first[k]), view(again[k])) and np.array_equal(view(flipped[k][::-1]), view(first[k]))
        assert np.array_equal(view(alone[k][0]), view(first[k][1]))
    print("two runs, a reversed batch and a row alone: the same bits")


def test_beyond_the_kernel_range_and_the_entry_point():
    """D = 65 is one feature more than the kernel takes: the stock-op path, on the device, is the emulation as well."""
    T_a, T_b, D = 20, 27, analysis.DTW_KERNEL_MAX_FEATURES + 1
    xa, xb = ref.sequences(2, T_a, T_b, D)
    want = [ref.dtw_fp32(xa[b], xb[b], 4, 0.01) for b in range(2)]
    worst = check(device(xa, xb, radius=4, penalty=0.01, timing=0.5), want, T_a, T_b, 0.5)
    print(f"D = {D}, the torch path on the device: the emulation's paths and costs; positions within {worst} ulp")
    assert worst <= 1
    L = ddsp._lib.lib()
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    call = lambda T_a=4, T_b=4, D=2, radius=0, penalty=0.0, nbytes=1 << 16: L.ddsp_dtw_align(                  # noqa: E731
        p, p, p, p, p, p, p, p, nbytes, 1, T_a, T_b, D, 4, radius, penalty, 0.0, torch.cuda.current_stream().cuda_stream)
    assert call(D=65) == -2 and call(T_a=2049) == -2 and call(T_b=2049) == -2
    assert call(radius=-1) == -1 and call(penalty=-1.0) == -1 and call(nbytes=8) == -1 and call(T_a=0) == -1
    empty = ddsp.dtw_align(torch.zeros(0, 4, 3, device="cuda"), torch.zeros(0, 5, 3, device="cuda"))
    assert empty[0].shape == (0, 4) and empty[0].is_cuda


def test_captured_in_a_graph():
    case = (2, 64, 65, 64, None, 0.0)
    xa, xb, want = emulation(case)
    a, b = cuda(xa), cuda(xb)
    ddsp.dtw_align(a, b)                                        # (the library is loaded outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ddsp.dtw_align(a, b, timing=0.5, return_path=True)
    graph.replay()
    torch.cuda.synchronize()
    worst = check([v.cpu().numpy() for v in out], want, 64, 65, 0.5)
    print(f"one launch, captured and replayed: the emulation's paths; positions within {worst} ulp")
    assert worst <= 1


def phrase_controls():
    A, w = ref.phrase()
    ctrl_a = dict(f0=cuda(A["f0"])[None, :, None], a=cuda(A["a"])[None, :, None], c=cuda(A["c"])[None], H=cuda(A["N"])[None])
    ctrl_b = ddsp.transform_controls(ctrl_a, SR, positions=cuda(w.astype(np.float32)), transpose=5.0, formant=0.0)
    return ctrl_a, ctrl_b, w


def test_a_phrase_aligns_with_its_slower_transposed_take():
    """The cap, not a measurement: every path point (i, j) has i and w(j) in one segment, and |i - w(j)| <= 1."""
    ctrl_a, ctrl_b, w = phrase_controls()
    for penalty in (0.0, 0.01):
        pos_a, pos_b, path, length, cost = ddsp.align_controls(ctrl_a, ctrl_b, SR, penalty=penalty, return_path=True)
        assert pos_a.is_cuda and path.is_cuda
        wrong, off = ref.phrase_deviation(path[0, :int(length[0])].cpu().numpy().astype(np.int64), w)
        print(f"penalty {penalty}: {int(length[0])} path points, {wrong} across segments, |i - w(j)| <= {off}, cost {float(cost[0]):.4f}")
        assert wrong == 0 and off <= 1


def formant_misses(out, T_out):
    """The output frames (of those where the phrase is voiced) whose largest harmonic lies more than one harmonic spacing from
    the phrase's formant at that frame."""
    f0 = out["f0"][0, :, 0].double().cpu().numpy()
    amp = (out["a"][0] * out["c"][0]).double().cpu().numpy()
    misses, frames = [], 0
    for t in range(T_out):
        centre = ref.phrase_formant(t)
        if centre is not None:
            frames += 1
            peak = (int(np.argmax(amp[t])) + 1) * f0[t]
            if not abs(peak - centre) <= f0[t]:
                misses.append(t)
    return misses, frames


def test_the_morph_of_an_aligned_phrase_keeps_its_formants():
    """Halfway in the harmonics between the phrase and its second take, on the phrase's clock: with the alignment the formant of
    every voiced frame is where the phrase has it; with the linear map a number of frames cross-fade two different segments."""
    ctrl_a, ctrl_b, _ = phrase_controls()
    pos_a, pos_b = ddsp.align_controls(ctrl_a, ctrl_b, SR, penalty=0.01, timing=0.0)
    assert torch.equal(pos_a[0], torch.arange(48.0, device="cuda"))
    aligned = ddsp.morph_controls(ctrl_a, ctrl_b, SR, mix_harmonics=0.5, positions_a=pos_a, positions_b=pos_b)
    linear = ddsp.morph_controls(ctrl_a, ctrl_b, SR, mix_harmonics=0.5)
    good, frames = formant_misses(aligned, 48)
    bad, _ = formant_misses(linear, 48)
    print(f"formant more than a harmonic spacing off: {len(good)} of {frames} voiced frames aligned, {len(bad)} with the linear map {bad}")
    assert frames == 40 and not good and len(bad) > 0


def test_autoencoder_morph_aligned():
    H, hop = AEConf.n_harmonics, AEConf.hop_length
    from control_morph_reference import formant_tone
    tones = [dict(zip(("f0", "a", "c"), formant_tone(T, H, f0, ((700.0, 150.0, 1.0), (1900.0, 250.0, 0.5))))) for T, f0 in ((44, 220.0), (60, 330.0))]
    ae = ddsp.AutoEncoder(AEConf, tracker='yin').cuda().eval()
    x, y = (ae.decoder.harmonics(dict(f0=cuda(s["f0"])[None, :, None], a=cuda(s["a"])[None, :, None], c=cuda(s["c"])[None])) for s in tones)
    assert x.shape[1] != y.shape[1]
    T_x, T_y = ae.analyse(x)["f0"].shape[1], ae.analyse(y)["f0"].shape[1]
    out = ae.morph(x, y, align=True)
    late = ae.morph(x, y, align=True, timing=1.0, radius=8, penalty=0.01)
    fixed = ae.morph(x, y, align=True, frames=50, noise=False)
    print(f"AutoEncoder.morph(align=True): {T_x} and {T_y} frames -> {out.shape[1] // hop}, {late.shape[1] // hop} and {fixed.shape[1] // hop}")
    assert out.shape == (1, T_x * hop) and late.shape == (1, T_y * hop) and fixed.shape == (1, 50 * hop)
    assert all(bool(torch.isfinite(v).all()) and float(v.abs().max()) > 0 for v in (out, late, fixed))
    with pytest.raises(ValueError, match="align"):
        ae.morph(x, y, align=True, positions_a=torch.zeros(T_x, device="cuda"))
    plain = ae.morph(x, y, mix=0.3, noise=False)
    assert torch.equal(ae.morph(x, y, mix=0.3, noise=False, align=False), plain)                   # what it was, bit for bit
