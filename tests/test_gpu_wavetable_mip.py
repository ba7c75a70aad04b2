"""The band-limited wavetable kernels (csrc/ddsp_wavetable_mip.hip, csrc/ddsp_wavetable.hip: *_bl) against
tests/wavetable_mip_reference.py, stage by stage, each stage fed exact fp32 inputs: the mip build, its adjoint, the forward and the
backward on the levels, then the module end to end.  The paths (levels staged in LDS / read from memory / a lowered LDS budget that
mixes both in one clip) are forced through ddsp_wavetable_set_form and ddsp_wavetable_set_mip_lds."""
import numpy as np
import pytest
import torch

import ddsp_pytorch_amd as ddsp
import wavetable_mip_reference as mip
import wavetable_reference as ref

pytestmark = pytest.mark.gpu

SR = 16000
BUILD_SHAPES = [(3, 16), (5, 64), (4, 512)]                                     # N, L
SHAPES = [(2, 6, 8, 5, 64), (3, 5, 64, 4, 16), (1, 4, 128, 33, 64)]             # B, T, hop, N, L
TRACKS = ("constant", "ramp", "octaves", "stall", "nyquist")
PATHS = ("lds", "global", "mixed")
GUARD, SENTINEL = 64, -12345.0
_CACHE = {}


@pytest.fixture(autouse=True)
def _default_hooks():
    yield
    L = ddsp._lib.lib()
    assert L.ddsp_wavetable_set_form(0) == 0 and L.ddsp_wavetable_set_grid(0) == 0 and L.ddsp_wavetable_set_mip_lds(0) == 0


def image_bytes(N, L):
    P4 = ((N + 3) // 4) | 1
    return 16 * (L * P4 + (L >> 4) + P4)


def set_path(path, shape, chunk_frames=0, iter_frames=0, backward=False):
    """'lds': every level staged (forced); 'global': none; 'mixed': a budget of three levels (beside the backward's records), so
    that a unit whose frames span more than that reads memory and the others stage."""
    B, T, hop, N, L = shape
    lib = ddsp._lib.lib()
    form = {"lds": 1, "global": 2, "mixed": 0}[path]
    assert lib.ddsp_wavetable_set_form(form | (chunk_frames << 8) | (iter_frames << 16)) == 0
    if path == "mixed":
        F = min(1024 // hop, T)
        F = min(F, iter_frames) if iter_frames else F
        assert lib.ddsp_wavetable_set_mip_lds(256 + 3 * image_bytes(N, L) + (32 * F * hop if backward else 0)) == 0
    plan = ddsp.wavetable_form_bl(B, T, N, L, hop)
    kind = "backward" if backward else "forward"
    assert plan[kind] == ("global" if path == "global" else "lds")
    assert plan[kind + "_fit"] == {"lds": mip.levels_of(L), "global": 0, "mixed": 3}[path]
    return plan


def f0_track(kind, B, T, L, rng):
    if kind == "constant":
        f0 = np.full((B, T), 220.0)
    elif kind == "ramp":                                    # crosses every level boundary, several of them inside one frame
        f0 = np.linspace(100.0, 7000.0, B * T).reshape(B, T)
    elif kind == "octaves":                                 # frames at exactly sample_rate 2^e / L: t = 0 exactly there
        e = rng.integers(0, int(np.log2(L)) - 1, (B, T))
        f0 = SR * 2.0 ** e / L
    elif kind == "stall":                                   # frames at exactly 0 Hz
        f0 = rng.uniform(100.0, 900.0, (B, T))
        f0[:, 1::2] = 0.0
    else:                                                   # a frame above sample_rate / 2
        f0 = rng.uniform(100.0, 900.0, (B, T))
        f0[:, T // 2] = 9000.0
    return f0.astype(np.float32)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def guarded(n):
    buf = torch.full((n + 2 * GUARD,), SENTINEL, device="cuda")
    return buf, buf[GUARD:GUARD + n]


def guards_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all() and (buf[-GUARD:] == SENTINEL).all())


def raw_build(W):
    N, L = W.shape
    n = mip.levels_of(L)
    buf, M = guarded(n * N * L)
    Wd, Dd = dev(W), dev(mip.dirichlet(L))
    assert ddsp._lib.lib().ddsp_wavetable_mip_build(Wd.data_ptr(), Dd.data_ptr(), M.data_ptr(), N, L, None) == 0
    torch.cuda.synchronize()
    assert guards_intact(buf)
    return M.cpu().numpy().reshape(n, N, L)


def raw_adjoint(G):
    n, N, L = G.shape
    buf, out = guarded(N * L)
    Gd, Dd = dev(G), dev(mip.dirichlet(L))
    assert ddsp._lib.lib().ddsp_wavetable_mip_adjoint(Gd.data_ptr(), Dd.data_ptr(), out.data_ptr(), N, L, None) == 0
    torch.cuda.synchronize()
    assert guards_intact(buf)
    return out.cpu().numpy().reshape(N, L)


def levels_for(N, L, seed=3):
    """fp32 levels to feed the synthesis stages: the reference's, rounded (exact inputs: the build's error stays in the build's test)"""
    key = (N, L, seed)
    if key not in _CACHE:
        W = np.random.default_rng(seed).standard_normal((N, L)).astype(np.float32)
        _CACHE[key] = (W, mip.build(W)[0].astype(np.float32))
    return _CACHE[key]


def make_case(shape, track, seed):
    B, T, hop, N, L = shape
    rng = np.random.default_rng(seed)
    W, M = levels_for(N, L)
    return dict(shape=shape, f0=f0_track(track, B, T, L, rng), c=rng.uniform(0.05, 2.0, (B, T, N)).astype(np.float32),
                a=rng.uniform(0.1, 1.5, (B, T)).astype(np.float32), W=W, M=M)


def raw_forward(case, phase=None):
    B, T, hop, N, L = case["shape"]
    f0, c, a, M = dev(case["f0"]), dev(case["c"]), dev(case["a"]), dev(case["M"])
    buf, y = guarded(B * T * hop)
    rc = ddsp._lib.lib().ddsp_wavetable_forward_bl(f0.data_ptr(), c.data_ptr(), a.data_ptr(), M.data_ptr(), y.data_ptr(),
                                                   None if phase is None else phase.data_ptr(), B, T, N, L, hop, SR, None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert guards_intact(buf)
    return y.cpu().numpy().reshape(B, T * hop)


def raw_backward(case, gy):
    B, T, hop, N, L = case["shape"]
    n = mip.levels_of(L)
    lib = ddsp._lib.lib()
    f0, c, a, M, g = dev(case["f0"]), dev(case["c"]), dev(case["a"]), dev(case["M"]), dev(gy.astype(np.float32))
    (bc, gc), (ba, ga), (bm, gm) = guarded(B * T * N), guarded(B * T), guarded(n * N * L)
    scratch = torch.empty(lib.ddsp_wavetable_backward_bl_scratch_bytes(B, T, N, L, hop), device="cuda", dtype=torch.uint8)
    rc = lib.ddsp_wavetable_backward_bl(g.data_ptr(), f0.data_ptr(), c.data_ptr(), a.data_ptr(), M.data_ptr(), None, scratch.data_ptr(),
                                        gc.data_ptr(), ga.data_ptr(), gm.data_ptr(), B, T, N, L, hop, SR, None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert guards_intact(bc) and guards_intact(ba) and guards_intact(bm)
    return gc.cpu().numpy().reshape(B, T, N), ga.cpu().numpy().reshape(B, T, 1), gm.cpu().numpy().reshape(n, N, L)


def check_forward(case, y, P0=None):
    want, bound, _ = mip.forward(case["f0"], case["c"], case["a"], case["M"], case["shape"][2], SR, P0)
    err = np.abs(y.astype(np.float64) - want)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"forward {case['shape']}: max err {err.max():.3e}, worst err / bound {worst:.3f}")
    assert np.isfinite(y).all() and (err <= bound).all(), worst


def check_backward(case, gy, got):
    want = mip.backward(gy, case["f0"], case["c"], case["a"], case["M"], case["shape"][2], SR)
    for name, g in zip(("c", "a", "M"), got):
        err = np.abs(g.astype(np.float64) - want["grad_" + name])
        bound = want["bound_" + name]
        worst = float((err / np.maximum(bound, 1e-300)).max())
        print(f"grad_{name} {case['shape']}: max err {err.max():.3e}, worst err / bound {worst:.3f}")
        assert np.isfinite(g).all() and (err <= bound).all(), (name, worst)


def unit_level_spans(case, chunk_frames):
    """levels a unit (row, chunk of chunk_frames frames) hears, from the reference's per-sample levels"""
    B, T, hop, N, L = case["shape"]
    q, q1, t = mip.level_weights(ref.increments(case["f0"], hop, SR), L)
    spans = []
    for b in range(B):
        for t0 in range(0, T, chunk_frames):
            sl = slice(t0 * hop, min(t0 + chunk_frames, T) * hop)
            spans.append(int(q1[b, sl].max() - q[b, sl].min() + 1))
    return spans


# ---- the build and its adjoint --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,L", BUILD_SHAPES)
def test_build_against_fp64(N, L):
    rng = np.random.default_rng(L + N)
    spike = np.zeros((N, L), np.float32)
    spike[0, L - 1] = 1.0                                   # one non-zero entry, at the wrap point
    for W in (rng.standard_normal((N, L)).astype(np.float32), spike):
        want, bound = mip.build(W)
        M = raw_build(W)
        err = np.abs(M.astype(np.float64) - want)
        print(f"build ({N}, {L}): max err {err.max():.3e}, worst err / bound {(err[1:] / np.maximum(bound[1:], 1e-300)).max():.3f}")
        assert (err <= bound).all()
        assert np.array_equal(M[0].view(np.uint32), W.view(np.uint32))          # level 0: bit for bit
        assert np.array_equal(M.view(np.uint32), raw_build(W).view(np.uint32))  # the same bits every run
    mean = want[-1]                                          # (the spike's top level: its mean, 1 / L in table 0)
    assert np.abs(mean[0] - 1.0 / L).max() <= 1e-9 and not mean[1:].any()


@pytest.mark.parametrize("N,L", BUILD_SHAPES)
def test_adjoint_against_fp64(N, L):
    rng = np.random.default_rng(7 * L + N)
    n = mip.levels_of(L)
    G = rng.standard_normal((n, N, L)).astype(np.float32)
    W = rng.standard_normal((N, L)).astype(np.float32)
    want, bound = mip.adjoint(G)
    got = raw_adjoint(G)
    err = np.abs(got.astype(np.float64) - want)
    print(f"adjoint ({N}, {L}): max err {err.max():.3e}, worst err / bound {(err / bound).max():.3f}")
    assert (err <= bound).all()
    assert np.array_equal(got.view(np.uint32), raw_adjoint(G).view(np.uint32))
    # <build(W), G> = <W, adjoint(G)> within the two bounds summed against the other factor
    M = raw_build(W)
    _, bound_M = mip.build(W)
    lhs = (M.astype(np.float64) * G).sum()
    rhs = (W.astype(np.float64) * got).sum()
    slack = (bound_M * np.abs(G)).sum() + (bound * np.abs(W)).sum()
    print(f"<build W, G> - <W, adjoint G> = {lhs - rhs:.3e}, allowed {slack:.3e}")
    assert abs(lhs - rhs) <= slack


# ---- the forward ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("shape", SHAPES)
def test_forward_against_fp64(shape, path):
    set_path(path, shape)
    for i, track in enumerate(TRACKS):
        case = make_case(shape, track, 100 + i)
        y = raw_forward(case)
        check_forward(case, y)
        if track == "ramp":
            assert all(np.array_equal(y, raw_forward(case)) for _ in range(2))  # the same bits every run


def test_lowered_budget_mixes_both_paths_in_one_clip():
    shape = (4, 6, 8, 5, 64)
    case = make_case(shape, "constant", 17)
    case["f0"][1] = np.linspace(100.0, 7000.0, 6)          # rows 1 and 3 sweep six levels, rows 0 and 2 stay inside two
    case["f0"][3] = np.linspace(7000.0, 100.0, 6)
    plan = set_path("mixed", shape)
    spans = unit_level_spans(case, 6)
    assert plan["forward_fit"] == 3 and min(spans) <= 3 < max(spans), spans
    y = raw_forward(case)
    check_forward(case, y)
    set_path("global", shape)
    assert np.array_equal(y, raw_forward(case))             # whichever path a unit takes, it reads the same numbers


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("chunk_frames,iter_frames", [(2, 1), (3, 2)])
def test_forward_chunk_prefix_and_carried_scan(path, chunk_frames, iter_frames):
    for shape in (SHAPES[0], SHAPES[1]):
        set_path(path, shape, chunk_frames, iter_frames)
        for track in ("ramp", "octaves"):
            case = make_case(shape, track, 7)
            check_forward(case, raw_forward(case))


@pytest.mark.parametrize("path", PATHS)
def test_grid_cap_strides_over_units(path):
    shape = (4, 4, 8, 5, 64)
    set_path(path, shape, 2, 1)
    assert ddsp._lib.lib().ddsp_wavetable_set_grid(2) == 0   # 4 rows x 2 chunks = 8 units on 2 workgroups
    case = make_case(shape, "ramp", 11)
    check_forward(case, raw_forward(case))
    set_path(path, shape, 2, 1, backward=True)
    gy = np.random.default_rng(12).standard_normal((4, 32))
    check_backward(case, gy, raw_backward(case, gy))


# ---- properties -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ("lds", "global"))
def test_below_half_an_entry_per_sample_is_the_unlimited_forward(path):
    """L = 64 and f0 <= 120 Hz: r <= 0.48, every sample reads level 0 alone -- the unlimited kernel's bits."""
    shape = (2, 6, 8, 5, 64)
    set_path(path, shape)
    case = make_case(shape, "constant", 31)
    case["f0"] = np.random.default_rng(32).uniform(0.0, 120.0, (2, 6)).astype(np.float32)
    y = raw_forward(case)
    f0, c, a, W = dev(case["f0"]), dev(case["c"]), dev(case["a"]), dev(case["W"])
    plain = torch.empty(2, 48, device="cuda")
    assert ddsp._lib.lib().ddsp_wavetable_forward(f0.data_ptr(), c.data_ptr(), a.data_ptr(), W.data_ptr(), plain.data_ptr(), None, None,
                                                  2, 6, 5, 64, 8, SR, None) == 0
    assert np.array_equal(y.view(np.uint32), plain.cpu().numpy().view(np.uint32))


def test_a_harmonic_above_nyquist_is_silent_and_below_a_quarter_untouched():
    """A table sin(2 pi h j / L).  Where every level heard has lost harmonic h, what is left of it is the build's error: |y| is
    within up(a) times the bound of the levels THE SAMPLE hears, blended as the sample blends them.  The bound of a level is taken
    as its largest element's (in the levels that lost the harmonic the bound is the same in every element to 0.2 %, and the
    position is the kernel's to compute), plus the level's own residue in the fp64 reference -- the fp32 rounding of the Dirichlet kernels, below
    1 % of the bound --, since the build promises its bound against the sum with those kernels, not against zero."""
    B, T, hop, N, L, h = 1, 6, 8, 1, 64, 8
    S = np.sin(2 * np.pi * h * np.arange(L) / L)[None].astype(np.float32)
    M = raw_build(S)                                        # (the device's own levels)
    want_M, bound_M = mip.build(S)
    n = mip.levels_of(L)
    lost = np.array([L >> (q + 1) < h for q in range(n)])   # levels 3 .. Q
    off_zero = np.array([(bound_M[q].max() + np.abs(want_M[q]).max()) if lost[q] else np.inf for q in range(n)])
    off_table = np.array([bound_M[q].max() + np.abs(want_M[q] - S).max() for q in range(n)])      # (level 0: 0)
    rng = np.random.default_rng(41)
    a = rng.uniform(0.1, 1.5, (B, T)).astype(np.float32)
    case = dict(shape=(B, T, hop, N, L), c=np.ones((B, T, N), np.float32), a=a, W=S, M=M)
    i0, i1, w0, w1 = ref.upsample_plan(T, hop)
    au = w0[None] * a[:, i0].astype(np.float64) + w1[None] * a[:, i1].astype(np.float64)
    blend = lambda per_level, q, q1, t: np.where(t > 0, (1.0 - t) * per_level[q] + t * per_level[q1], per_level[q])   # noqa: E731
    # h f0 > sample_rate / 2: every level heard has lost harmonic 8
    case["f0"] = rng.uniform(1010.0, 7000.0, (B, T)).astype(np.float32)
    y = raw_forward(case)
    q, q1, t = mip.level_weights(ref.increments(case["f0"], hop, SR), L)
    assert lost[q].all() and q.min() >= 3
    allowed = blend(off_zero, q, q1, t) * au
    print(f"above Nyquist: max |y| {np.abs(y).max():.3e}, worst |y| / allowed {(np.abs(y) / allowed).max():.3f}")
    assert (np.abs(y) <= allowed).all()
    # 2 h f0 <= sample_rate / 2: both levels heard still hold harmonic 8 -- the unlimited output within the sum of the bounds
    case["f0"] = rng.uniform(60.0, 499.0, (B, T)).astype(np.float32)
    y = raw_forward(case)
    q, q1, t = mip.level_weights(ref.increments(case["f0"], hop, SR), L)
    assert (~lost[q]).all() and (~lost[q1] | (t == 0)).all()
    want, bound, _ = ref.forward(case["f0"], case["c"], a, S, hop, SR)
    _, bound_bl, _ = mip.forward(case["f0"], case["c"], a, M, hop, SR)
    assert (np.abs(y - want) <= bound + bound_bl + blend(off_table, q, q1, t) * au).all()


# ---- the backward ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("shape", SHAPES)
def test_backward_against_fp64(shape, path):
    set_path(path, shape, backward=True)
    B, T, hop, N, L = shape
    rng = np.random.default_rng(50)
    for i, track in enumerate(("ramp", "octaves", "stall", "nyquist")):
        case = make_case(shape, track, 60 + i)
        case["c"][0, T // 2] = 0.7                           # a frame whose c is all equal: the normalisation's term alone
        gy = rng.standard_normal((B, T * hop))
        got = raw_backward(case, gy)
        check_backward(case, gy, got)
        if i == 0:
            again = raw_backward(case, gy)
            assert np.array_equal(got[0], again[0]) and np.array_equal(got[1], again[1])        # grad_c, grad_a: the same bits
    one = np.zeros((B, T * hop))                             # one sample: every scatter target can be read off
    one[B - 1, (T * hop) // 2 + 1] = 1.5
    check_backward(case, one, raw_backward(case, one))


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("chunk_frames,iter_frames", [(2, 1), (3, 2)])
def test_backward_chunk_prefix_and_carried_scan(path, chunk_frames, iter_frames):
    for shape in (SHAPES[0], SHAPES[1]):
        set_path(path, shape, chunk_frames, iter_frames, backward=True)
        case = make_case(shape, "ramp", 71)
        gy = np.random.default_rng(72).standard_normal((shape[0], shape[1] * shape[2]))
        check_backward(case, gy, raw_backward(case, gy))


# ---- end to end -----------------------------------------------------------------------------------------------------------------
def bank(shape, W, band_limited=True):
    class Conf:
        n_harmonics, sample_rate, hop_length = shape[3], SR, shape[2]
    return ddsp.WavetableBank(Conf, table_size=shape[4], init=torch.from_numpy(W), band_limited=band_limited).cuda()


def test_autograd_equals_the_chain_of_raw_calls():
    shape = SHAPES[0]
    B, T, hop, N, L = shape
    case = make_case(shape, "ramp", 80)
    wt = bank(shape, case["W"])
    f0, c, a = dev(case["f0"][..., None]), dev(case["c"]).requires_grad_(), dev(case["a"][..., None]).requires_grad_()
    gy = np.random.default_rng(81).standard_normal((B, T * hop)).astype(np.float32)
    M = ddsp.wavetable_mipmaps(wt.wavetables.detach())
    assert torch.equal(M[0], wt.wavetables.detach()) and np.array_equal(M.cpu().numpy(), raw_build(case["W"]))
    y = wt({"f0": f0, "c": c, "a": a})
    assert torch.equal(y, ddsp.wavetable_forward_bl(f0, c, a, M, hop, SR))
    y.backward(dev(gy))
    gc, ga, gM = ddsp.wavetable_backward_bl(dev(gy), f0, c, a, M, hop, SR)
    assert torch.equal(c.grad, gc) and torch.equal(a.grad, ga)                   # bitwise
    # grad_W: the adjoint of the device's grad_M against fp64, plus what grad_M's own bound becomes through the adjoint
    dev_case = dict(case, M=M.cpu().numpy())
    want = mip.backward(gy, case["f0"], case["c"], case["a"], dev_case["M"], hop, SR)
    gW, bound_adj = mip.adjoint(want["grad_M"])
    carried, _ = mip.adjoint(want["bound_M"], np.abs(mip.dirichlet(L)))
    err = np.abs(wt.wavetables.grad.cpu().numpy().astype(np.float64) - gW)
    print(f"grad_W: max err {err.max():.3e}, worst err / bound {(err / (bound_adj + carried)).max():.3f}")
    assert (err <= bound_adj + carried).all()
    # and the switch off is the unlimited module, bit for bit
    off = bank(shape, case["W"], band_limited=False)
    with torch.no_grad():
        assert torch.equal(off({"f0": f0, "c": c, "a": a}), ddsp.wavetable_forward(f0, c, a, off.wavetables, hop, SR))


def test_live_blocks_equal_one_forward_and_carry_the_phase():
    """Two live blocks against one forward over the whole clip, to the bit.  What makes that possible: the two frames at the cut
    hold the same controls (a block clamps its interpolation at its own edge), and every f0 is a multiple of sample_rate / 1024 at
    hop 16, so that the increments and their fp64 sums are exact whichever way a call groups them."""
    shape = (3, 8, 16, 5, 64)
    B, T, hop, N, L = shape
    case = make_case(shape, "constant", 30)
    steps = np.array([[8, 20, 33, 47, 47, 90, 160, 290], [3, 5, 9, 17, 17, 30, 41, 64], [440, 300, 200, 120, 120, 60, 30, 11]])
    case["f0"] = (steps * (SR / 1024.0)).astype(np.float32)                      # 47 Hz .. 6875 Hz: every level but the top
    case["c"][:, 4], case["a"][:, 4] = case["c"][:, 3], case["a"][:, 3]
    wt = bank(shape, case["W"])
    case["M"] = wt.levels().cpu().numpy()
    x = {"f0": dev(case["f0"][..., None]), "c": dev(case["c"]), "a": dev(case["a"][..., None])}
    with torch.no_grad():
        whole = wt(x)
        blocks = [wt.live({k: v[:, 4 * i:4 * i + 4].contiguous() for k, v in x.items()}) for i in range(2)]
    check_forward(case, whole.cpu().numpy())
    assert torch.equal(torch.cat(blocks, dim=1), whole)
    end = ref.phases(case["f0"], hop, SR)[:, -1] % 1.0
    state = wt.phase.cpu().numpy()
    assert np.array_equal(state, end) and len(set(state.tolist())) == B          # exact, and every row its own
    # a second pass goes on from the carried phase: the reference started there
    with torch.no_grad():
        again = wt.live(x)
    check_forward(case, again.cpu().numpy(), end)
    assert not torch.equal(again, whole)
    wt.reset_phase()
    with torch.no_grad():
        assert torch.equal(wt.live(x), whole) and float(wt.phase.abs().max()) > 0.0


def test_live_under_graph_replay_equals_eager_and_the_pyramid_follows_the_tables():
    shape = (2, 4, 16, 5, 64)
    B, T, hop, N, L = shape
    case = make_case(shape, "ramp", 41)
    x = {"f0": dev(case["f0"][..., None]), "c": dev(case["c"]), "a": dev(case["a"][..., None])}
    wt = bank(shape, case["W"])
    with torch.no_grad():
        eager = [wt.live(x).clone() for _ in range(2)]
        levels = wt.levels()
        assert wt.levels() is levels                         # cached: a live block is one launch
        wt.reset_phase()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            wt.live(x)
        torch.cuda.current_stream().wait_stream(side)
        wt.reset_phase()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = wt.live(x)
        wt.reset_phase()
        for want in eager:
            graph.replay()
            assert torch.equal(out, want)
    # after an optimiser step the cached pyramid is rebuilt: the output changes, and equals a fresh module's on the new tables
    opt = torch.optim.SGD(wt.parameters(), lr=0.5)
    wt(x).square().sum().backward()
    opt.step()
    assert wt.levels() is not levels and torch.equal(wt.levels()[0], wt.wavetables.detach())
    wt.reset_phase()
    with torch.no_grad():
        after = wt.live(x)
        fresh = bank(shape, wt.wavetables.detach().cpu().numpy()).live(x)
    assert not torch.equal(after, eager[0]) and torch.equal(after, fresh)


class TinyConf:
    n_harmonics, n_noise_filters, sample_rate, hop_length = 8, 65, SR, 64
    decoder_mlp_units, decoder_mlp_layers, decoder_gru_units, decoder_gru_layers = 256, 1, 32, 1
    wavetable_size = 64


def tiny_batch(B=2, T=8, seed=90):
    g = torch.Generator().manual_seed(seed)
    return {"f0": (100 + 300 * torch.rand(B, T, 1, generator=g)).cuda(), "normalized_cents": torch.rand(B, T, 1, generator=g).cuda(),
            "loudness": torch.rand(B, T, 1, generator=g).cuda(), "audio": (0.1 * torch.randn(B, T * 64, generator=g)).cuda()}


def tiny_decoder():
    torch.manual_seed(5)
    return ddsp.Decoder(TinyConf, noise_rng="device", seed=3, synth="wavetable", band_limited=True).cuda()


def test_decoder_trains_with_falling_loss():
    dec, batch = tiny_decoder(), tiny_batch()
    assert dec.harmonics.band_limited and dec.harmonics.wavetables.shape == (8, 64)
    loss_fn = ddsp.MSSLoss((256, 128, 64)).cuda()
    opt = torch.optim.Adam(dec.parameters(), lr=1e-3)
    before = dec.harmonics.wavetables.detach().clone()
    losses = []
    for _ in range(3):
        out = ddsp.train_step(dec, loss_fn, opt, batch)
        losses.append(float(out[0] if isinstance(out, (tuple, list)) else out))
    print("losses", losses)
    assert all(np.isfinite(v) for v in losses) and losses[2] < losses[0]
    assert not torch.equal(before, dec.harmonics.wavetables.detach())
    with torch.no_grad():
        assert dec(batch).shape == (2, 8 * 64) and bool(torch.isfinite(dec(batch)).all())


def test_graphed_train_step_replays_and_every_later_call_plays_the_trained_tables():
    """A replayed optimiser update rewrites the tables without touching the parameter's version counter.  Whatever ran before the
    replays -- a no-grad forward, a live block (which caches the levels) --, a call after them plays the tables as they are."""
    dec, batch = tiny_decoder(), tiny_batch()
    wt = dec.harmonics
    ctl = {"f0": batch["f0"], "c": torch.rand(2, 8, 8, device="cuda") + 0.1, "a": torch.rand(2, 8, 1, device="cuda") + 0.1}
    with torch.no_grad():
        early = dec(batch).clone()                           # a no-grad call, and a live block, before anything is captured
        early_live = wt.live(ctl).clone()
    stale = wt.levels()
    loss_fn = ddsp.MSSLoss((256, 128, 64)).cuda()
    opt = torch.optim.Adam(dec.parameters(), lr=1e-2, capturable=True)
    step = ddsp.GraphedTrainStep(dec, loss_fn, opt, batch)
    before = wt.wavetables.detach().clone()
    losses = [float(step(batch)[0]) for _ in range(2)]
    assert all(np.isfinite(v) for v in losses)
    assert not torch.equal(before, wt.wavetables.detach())

    def fresh_bank():
        return ddsp.WavetableBank(TinyConf, band_limited=True, init=wt.wavetables.detach().cpu()).cuda()
    with torch.no_grad():
        assert torch.equal(wt(ctl), fresh_bank()(ctl))       # the module's no-grad forward: the current tables
        wt.reset_phase()
        after_live = wt.live(ctl)
        assert torch.equal(after_live, fresh_bank().live(ctl)) and not torch.equal(after_live, early_live)
        assert wt.levels() is not stale and torch.equal(wt.levels()[0], wt.wavetables.detach())
        # the whole decoder against a copy of it whose synthesiser is a fresh module on the current tables
        other = tiny_decoder()
        other.load_state_dict(dec.state_dict())
        dec.noise.reseed(3, 0)                               # (the same noise draw in both)
        other.noise.reseed(3, 0)
        out, want = dec(batch), other(batch)
    assert torch.equal(out, want) and not torch.equal(out, early)
