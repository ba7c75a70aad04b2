"""The GRU reference of tests/gru_reference.py, checked on the CPU: against fp64 autograd of a plain GRU, its `plan` against the
table of kernel instantiations in tests/test_gru.py, and -- the evidence that the GPU tests would fail on a subtly wrong kernel -- a
plain-torch fp32 emulation of the bf16 kernels that passes the criterion while seven seeded mutants of it fail."""
import pytest
import torch

import gru_reference as R


# ---- reference vs fp64 autograd -------------------------------------------------------------------------------------
def _plain_gru(gi, w, b, h0):
    B, T, G3 = gi.shape
    Hd = G3 // 3
    h = torch.zeros((B, Hd), dtype=gi.dtype) if h0 is None else h0
    ys, hps = [], []
    for t in range(T):
        gh = h @ w.T if b is None else h @ w.T + b
        r = torch.sigmoid(gi[:, t, :Hd] + gh[:, :Hd])
        z = torch.sigmoid(gi[:, t, Hd:2 * Hd] + gh[:, Hd:2 * Hd])
        n = torch.tanh(gi[:, t, 2 * Hd:] + r * gh[:, 2 * Hd:])
        hps.append(h)
        h = (1.0 - z) * n + z * h
        ys.append(h)
    return torch.stack(ys, 1), torch.stack(hps, 1)


@pytest.mark.parametrize("B,T,Hd,with_h0,with_bias", [(4, 5, 12, True, True), (3, 6, 33, False, True), (5, 4, 20, True, False),
                                                     (3, 1, 12, True, True), (2, 1, 9, False, False), (3, 7, 16, False, False)])
def test_unrounded_reference_at_its_fixed_point_equals_fp64_autograd(B, T, Hd, with_h0, with_bias):
    x = {k: (None if v is None else v.double()) for k, v in R.make_inputs(B, T, Hd, 100 + T + Hd, with_h0, with_bias).items()}
    gi = x["gi"].clone().requires_grad_()
    w = x["w"].clone().requires_grad_()
    h0 = None if x["h0"] is None else x["h0"].clone().requires_grad_()
    y_ag, hp_ag = _plain_gru(gi, w, x["b"], h0)
    ((y_ag * x["dy"]).sum() + (y_ag[:, -1] * x["dhT"]).sum()).backward()
    # forward: T passes from zeros, each feeding its own y back in, reach the recurrence's fixed point
    y = torch.zeros((B, T, Hd), dtype=torch.float64)
    for _ in range(T):
        y, r, z, n, ghn = R.forward_steps(x["gi"], x["w"], x["b"], x["h0"], y, torch.float64, False)
    assert float((y - y_ag.detach()).abs().max()) <= 1e-12
    gates = torch.cat((r, z, n), -1)
    d_gh = torch.zeros((B, T, 3 * Hd), dtype=torch.float64)
    for _ in range(T + 1):      # pass i makes d_gh exact for the last i steps; dh0 reads d_gh[0], exact after T passes: one more
        d_gi, d_gh, dh0 = R.backward_steps(x["dy"], x["dhT"], x["w"], x["h0"], y, gates, ghn, d_gh, torch.float64, False)
    assert float((d_gi - gi.grad).abs().max()) <= 1e-12
    if h0 is not None:
        assert float((dh0 - h0.grad).abs().max()) <= 1e-12
    dw = d_gh.reshape(B * T, 3 * Hd).T @ hp_ag.detach().reshape(B * T, Hd)
    assert float((dw - w.grad).abs().max()) <= 1e-12
    # dhT = None is a zero dhT
    a = R.backward_steps(x["dy"], None, x["w"], x["h0"], y, gates, ghn, d_gh, torch.float64, False)
    b = R.backward_steps(x["dy"], torch.zeros_like(x["dhT"]), x["w"], x["h0"], y, gates, ghn, d_gh, torch.float64, False)
    assert all(torch.equal(p, q) for p, q in zip(a, b))


# ---- plan() vs the source -------------------------------------------------------------------------------------------
# tests/test_gru.py:30-43 on 256 CUs: hd -> (KP, NW, slots), and (B -> BL) of the rows named there
_TABLE = {12: (4, 1, 256, {2: 1, 3: 1}),
          64: (4, 4, 64, {4: 1, 70: 2, 200: 4, 330: 6}),
          100: (8, 7, 32, {5: 1, 40: 2, 100: 4, 160: 5}),
          128: (8, 8, 32, {200: 7}),
          200: (16, 13, 16, {9: 1, 20: 2, 50: 4, 80: 5}),
          512: (32, 32, 8, {1: 1, 6: 1, 20: 3, 32: 4, 40: 5, 100: 13})}


def test_plan_reproduces_the_table_of_instantiations():
    for hd, (KP, NW, slots, rows) in _TABLE.items():
        assert R.resident_slots(256, NW, False) == slots
        for B, BL in rows.items():
            for lowp in (False, True):
                for backward in (False, True):
                    (s,) = R.plan(B, hd, 256, lowp, backward)
                    assert (s.rows, s.BL, s.KP, s.NW) == (B, BL, KP, NW), (hd, B, lowp, backward, s)
                    assert s.mfma == (lowp and (backward or BL >= 2))
                    if not s.mfma and not backward:
                        assert (s.RT, s.NRS) == (2, 1 if BL <= 2 else 2)
                    if not s.mfma and backward:
                        assert (s.RT, s.NRS) == ((2, 1) if BL <= 2 else (4, 1) if BL <= 4 else (2, 2))
    # 250 rows of 200 units: 16 per group in the fp32 forward; slices of 240 + 10 rows (15 + 1 per group) in the others
    (s,) = R.plan(250, 200, 256, False, False)
    assert (s.BL, s.NG, s.last, s.kernel) == (16, 16, 10, "gru_fwd_kernel<16,2,2>")
    for lowp, backward in ((False, True), (True, False), (True, True)):
        a, b = R.plan(250, 200, 256, lowp, backward)
        assert (a.rows, a.BL, a.NG, b.rows, b.BL, b.NG) == (240, 15, 16, 10, 1, 10)
    a, b = R.plan(250, 200, 256, True, False)
    assert (a.kernel, b.kernel) == ("gru_fwd_mfma_kernel<16>", "gru_fwd_kernel<16,2,1>")       # one row per group: the fp32 forward
    assert R.rounded_rows([a, b]).tolist() == [True] * 240 + [False] * 10
    # 150 rows of 512 units: 19 per group forward, slices of 112 + 38 rows (14 + 5 per group) backward
    (s,) = R.plan(150, 512, 256, False, False)
    assert (s.BL, s.NG, s.last) == (19, 8, 17)
    a, b = R.plan(150, 512, 256, False, True)
    assert (a.rows, a.BL, a.NG, a.kernel, b.rows, b.BL, b.NG, b.kernel) == (112, 14, 8, "gru_bwd_kernel<32,2,2>", 38, 5, 8, "gru_bwd_kernel<32,2,2>")
    # the tail slice of one row, the largest groups, the 16-bit epoch limit, the spread placement
    a, b = R.plan(113, 512, 256, True, False)
    assert (a.rows, a.mfma, b.rows, b.BL, b.mfma) == (112, True, 1, 1, False)
    (s,) = R.plan(1008, 64, 256, True, True)
    assert (s.BL, s.NG, s.last) == (16, 63, 16)
    assert R.plan(2, 12, 256, True, True, T=65535)[0].kernel == "gru_bwd_mfma_kernel<4>"
    assert R.plan(2, 12, 256, True, True, T=65536)[0].kernel == "gru_bwd_kernel<4,2,1>"
    assert [(s.BL, s.NG) for s in R.plan(14, 512, 256, True, False, spread=True)] == [(2, 7)]
    assert [(s.BL, s.NG) for s in R.plan(40, 200, 256, True, True, spread=True)] == [(3, 14)]
    with pytest.raises(ValueError):
        R.plan(4, 513, 256, False, False)


# ---- the comparison discriminates -----------------------------------------------------------------------------------
def _bf16(x):
    return x.to(torch.bfloat16).float()


def _trunc(x):
    return (x.contiguous().view(torch.int32) & -65536).view(torch.float32)


MUT_ROW, MUT_UNIT, MUT_STEP = 2, 3, 3        # a plain row (0 is saturated, 1 is zero), and the step that consumes the wrong value


def emulate(x, mutant=None):
    """The bf16 kernels in plain fp32 torch, running freely over the steps, with the kernels' rounding points: bf16(h_{t-1}) and
    bf16(W) in the forward product, bf16(d_gh) and bf16(W) in the backward one, everything else fp32.  `mutant` seeds one bug."""
    gi, w, b, h0, dy, dhT = (x[k] for k in ("gi", "w", "b", "h0", "dy", "dhT"))
    B, T, G3 = gi.shape
    Hd = G3 // 3
    wq = w.clone() if mutant == "w_unrounded" else _bf16(w)
    wf, wb = wq.clone(), wq.clone()
    if mutant == "k_block":                     # one 8-wide k-block of one unit (forward) / one column (backward) dropped
        for g in range(3):
            wf[g * Hd + MUT_UNIT, 0:8] = 0.0
            wb[g * Hd:g * Hd + 8, MUT_UNIT] = 0.0
    h = torch.zeros((B, Hd)) if h0 is None else h0.clone()
    imgs, ys, rs, zs, ns, hns = [], [], [], [], [], []
    for t in range(T):
        img = _trunc(h) if mutant == "h_trunc" else _bf16(h)
        imgs.append(img.clone())
        if t == MUT_STEP and mutant == "stale":
            img[MUT_ROW, MUT_UNIT] = imgs[t - 1][MUT_ROW, MUT_UNIT]                       # the image of h_{t-2}
        if t == MUT_STEP and mutant == "swap":
            img[[MUT_ROW, MUT_ROW + 1], MUT_UNIT] = img[[MUT_ROW + 1, MUT_ROW], MUT_UNIT]
        gh = img @ wf.T
        if b is not None:
            gh = gh + b
        r = torch.sigmoid(gi[:, t, :Hd] + gh[:, :Hd])
        z = torch.sigmoid(gi[:, t, Hd:2 * Hd] + gh[:, Hd:2 * Hd])
        ghn = gh[:, 2 * Hd:]
        n = torch.tanh(gi[:, t, 2 * Hd:] + r * ghn)
        hp, h = h, None
        h = n + z * (hp - n)
        for lst, v in zip((ys, rs, zs, ns, hns), (h, r, z, n, ghn)):
            lst.append(v)
    y, r, z, n, hn = (torch.stack(v, 1) for v in (ys, rs, zs, ns, hns))
    hT = y[:, -2].clone() if mutant == "hT_stale" else y[:, -1].clone()
    gates = torch.cat((r, z, n), -1)
    # backward, on the forward's own saved tensors
    hp = R.h_prev(h0, y, torch.float32)
    f_n = (1.0 - z) * (1.0 - n * n)
    f_r = (f_n * hn) * (r * (1.0 - r))
    f_z = (hp - n) * (z * (1.0 - z))
    f_hn = f_n * r
    carry = torch.zeros((B, Hd)) if dhT is None else dhT.clone()
    d_gi, d_gh = torch.empty((B, T, G3)), torch.empty((B, T, G3))
    pubs = []
    for s in range(T):
        t = T - 1 - s
        dh = dy[:, t] + carry
        a, c = dh * f_r[:, t], dh * f_z[:, t]
        d_gi[:, t] = torch.cat((a, c, dh * f_n[:, t]), -1)
        d_gh[:, t] = torch.cat((a, c, dh * f_hn[:, t]), -1)
        pub = d_gh[:, t].clone() if mutant == "published_unrounded" else _bf16(d_gh[:, t])
        pubs.append(pub.clone())
        cols = [MUT_UNIT, Hd + MUT_UNIT, 2 * Hd + MUT_UNIT]                                # the three payloads of one granule
        if s == MUT_STEP and mutant == "stale":
            pub[MUT_ROW, cols] = pubs[s - 2][MUT_ROW, cols]
        if s == MUT_STEP and mutant == "swap":
            for cidx in cols:
                pub[[MUT_ROW, MUT_ROW + 1], cidx] = pub[[MUT_ROW + 1, MUT_ROW], cidx]
        carry = dh * z[:, t] + pub @ wb
    return dict(y=y, hT=hT, gates=gates, hn=hn, d_gi=d_gi, d_gh=d_gh, dh0=carry)


def _verdict(x, out):
    T = out["y"].shape[1]
    fwd = R.forward_measures(x, out["y"], out["hT"], out["gates"], out["hn"], True)
    bwd = R.backward_measures(x, out["y"], out["gates"], out["hn"], out["d_gi"], out["d_gh"], out["dh0"], True)
    return fwd, bwd, R.failures(fwd, T), R.failures(bwd, T)


SHAPES = [(4, 6, 12), (5, 6, 200), (16, 8, 512)]       # B, T, Hd


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: f"B{s[0]}-T{s[1]}-Hd{s[2]}")
def case(request):
    B, T, Hd = request.param
    return R.make_inputs(B, T, Hd, 7 * Hd + B)


def test_fp32_emulation_of_the_bf16_kernels_passes_the_criterion(case):
    out = emulate(case)
    fwd, bwd, bad_f, bad_b = _verdict(case, out)
    print("forward ", R.describe(fwd))
    print("backward", R.describe(bwd))
    assert not bad_f and not bad_b, (bad_f, bad_b)
    assert torch.equal(out["hT"], out["y"][:, -1])
    # ... and not by a hair: given the previous outputs, a step of the emulation is a step of the fp32 reference (ratio ~ 1)
    assert R.worst_ratio(fwd) <= 2.0 and R.worst_ratio(bwd) <= 2.0


# mutant -> the directions whose check must fail
MUTANTS = {"h_trunc": ("forward",), "w_unrounded": ("forward", "backward"), "published_unrounded": ("backward",),
           "stale": ("forward", "backward"), "swap": ("forward", "backward"), "k_block": ("forward", "backward"), "hT_stale": ("forward",)}


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_every_seeded_mutant_fails_the_criterion(case, mutant):
    out = emulate(case, mutant)
    fwd, bwd, bad_f, bad_b = _verdict(case, out)
    exceeded = {"forward": [m for m in bad_f if "error" in m], "backward": [m for m in bad_b if "error" in m]}
    print(mutant, "forward ", R.describe(fwd))
    print(mutant, "backward", R.describe(bwd))
    for direction in MUTANTS[mutant]:
        assert exceeded[direction], (mutant, direction)
        # two orders of magnitude above the bound, not a near miss
        worst = R.worst_ratio(fwd if direction == "forward" else bwd)
        assert worst >= 100.0 * R.MARGIN, (mutant, direction, worst)
    if mutant == "hT_stale":
        assert not torch.equal(out["hT"], out["y"][:, -1])
