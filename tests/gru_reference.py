"""TEST INFRASTRUCTURE ONLY -- fp64 reference of the GRU recurrence (csrc/ddsp_gru.hip), one step at a time, and its criterion.

The recurrence of the bf16 matrix-core kernels rounds h to bf16 at every step, so two correct implementations drift apart by bf16
ulps as soon as one rounding falls the other way: a run-to-run comparison cannot be tighter than that drift.  This reference is
TEACHER-FORCED instead: every step is evaluated from the kernel's own previous output, the rounding is applied to the kernel's own
bits, and what is left is the arithmetic of one step -- fp32 round-off.  By induction (h0 correct, every step correct given the
previous outputs) the whole recurrence is correct, and a wrong, stale or misplaced hand-off value shows at the step that consumed it.

The kernels' semantics (`rounded=True`: the bf16 kernels; `rounded=False`: the fp32 kernels round neither h nor W):
    forward    gh_t = bf16(h_{t-1}) bf16(W_hh)^T + b_hh         (the product only; fp32 accumulation)
               r = s(gi_r + gh_r), z = s(gi_z + gh_z), n = tanh(gi_n + r gh_n), h_t = n + z (h_{t-1} - n)     unrounded fp32 values
    backward   dh_t = dy_t + z_{t+1} dh_{t+1} + bf16(d_gh_{t+1}) bf16(W_hh)
               d_gh_t = dh_t (f_r, f_z, f_hn), d_gi_t = dh_t (f_r, f_z, f_n)   with derive_step's five fp32 factors;
               the fp32 d_gh stores are the unrounded values whose bf16 image is what was handed on.

`forward_steps` takes h_{t-1} from the kernel's `y` (one matmul over all steps); `backward_steps` takes the product term from the
kernel's `d_gh` (one matmul) and carries the direct path z dh itself (a short linear scan over T, in NumPy: 65 535 steps of a [2, 12]
problem stay well under a second).  `dtype=torch.float32` evaluates the same formulas in fp32: the yardstick `e32` of the criterion.
`plan` restates plan_gru / resident_slots / ddsp_gru_max_batch / run_gru's choice of kernel, so that a test can state and assert
which instantiation and which rounding each batch row gets.

Nothing under ddsp-pytorch_amd/ may import this module.
"""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np
import torch

MARGIN = 8.0            # the kernel must be within MARGIN x e32 (see `failures`)
GAP_FACTOR = 32.0       # ... and MARGIN x e32 must be at most 1 / GAP_FACTOR of the distance between the two roundings


def bf16_round(x, dtype=torch.float64):
    """Round-to-nearest-even to bf16 of fp32 values, returned in `dtype` (what the kernels' (__bf16) conversions do)."""
    return x.to(torch.float32).to(torch.bfloat16).to(dtype)


def _cpu(x, dtype):
    return None if x is None else x.detach().cpu().to(dtype)


def _rows(rounded, B: int):
    """`rounded` as one flag per batch row: a bool, or a sequence / tensor of B bools."""
    if isinstance(rounded, (bool, int, np.bool_)):
        return torch.full((B,), bool(rounded))
    rows = torch.as_tensor(rounded, dtype=torch.bool).reshape(-1)
    assert rows.numel() == B, (rows.numel(), B)
    return rows


def h_prev(h0, y, dtype=torch.float64):
    """h_{t-1} of every step [B,T,Hd]: cat(h0 | 0, y[:, :-1])."""
    y = _cpu(y, dtype)
    first = torch.zeros_like(y[:, :1]) if h0 is None else _cpu(h0, dtype).unsqueeze(1)
    return torch.cat((first, y[:, :-1]), dim=1)


def forward_steps(gi, w_hh, b_hh, h0, y, dtype=torch.float64, rounded=True):
    """Every step of the forward from the kernel's own previous output.  gi [B,T,3Hd], w_hh [3Hd,Hd], b_hh [3Hd] | None,
    h0 [B,Hd] | None, y [B,T,Hd] (the kernel's) -> (h, r, z, n, ghn), each [B,T,Hd] in `dtype`; ghn = W_hn h_{t-1} + b_hn."""
    B, T, Hd = y.shape
    rows = _rows(rounded, B)
    gi, w = _cpu(gi, dtype), _cpu(w_hh, dtype)
    hp = h_prev(h0, y, dtype)
    gh = torch.empty((B, T, 3 * Hd), dtype=dtype)
    for flag in (True, False):
        idx = rows == flag
        if idx.any():
            gh[idx] = (bf16_round(hp[idx], dtype) @ bf16_round(w, dtype).T) if flag else (hp[idx] @ w.T)
    if b_hh is not None:
        gh = gh + _cpu(b_hh, dtype)
    r = torch.sigmoid(gi[..., :Hd] + gh[..., :Hd])
    z = torch.sigmoid(gi[..., Hd:2 * Hd] + gh[..., Hd:2 * Hd])
    ghn = gh[..., 2 * Hd:].contiguous()
    n = torch.tanh(gi[..., 2 * Hd:] + r * ghn)
    h = n + z * (hp - n)
    return h, r, z, n, ghn


def backward_steps(dy, dhT, w_hh, h0, y, gates, hn, d_gh, dtype=torch.float64, rounded=True):
    """Every step of the backward: the product term from the kernel's own `d_gh` (bf16-rounded where `rounded`; a bf16 `d_gh` -- io16 --
    is taken as it is), the direct path from the reference itself.  dy [B,T,Hd], dhT [B,Hd] | None, gates [B,T,3Hd] = r|z|n and
    hn [B,T,Hd] as the forward saved them -> (d_gi [B,T,3Hd], d_gh [B,T,3Hd], dh0 [B,Hd]) in `dtype`."""
    B, T, Hd = y.shape
    rows = _rows(rounded, B)
    w = _cpu(w_hh, dtype)
    g = _cpu(gates, dtype)
    r, z, n = g[..., :Hd], g[..., Hd:2 * Hd], g[..., 2 * Hd:]
    ghn, hp = _cpu(hn, dtype), h_prev(h0, y, dtype)
    f_n = (1.0 - z) * (1.0 - n * n)               # derive_step, in its order
    f_r = (f_n * ghn) * (r * (1.0 - r))
    f_z = (hp - n) * (z * (1.0 - z))
    f_hn = f_n * r
    d = d_gh.detach().cpu()
    P = torch.empty((B, T, Hd), dtype=dtype)      # P[t] = q(d_gh[t]) q(W): what step t hands to step t-1
    for flag in (True, False):
        idx = rows == flag
        if idx.any():
            dq = d[idx].to(dtype) if (d.dtype == torch.bfloat16 or not flag) else bf16_round(d[idx], dtype)
            P[idx] = dq @ (bf16_round(w, dtype) if flag else w)
    npdt = np.float64 if dtype == torch.float64 else np.float32
    tm = lambda x: np.ascontiguousarray(x.numpy().transpose(1, 0, 2))      # noqa: E731  time-major [T,B,Hd]
    dy_t, z_t, P_t = tm(_cpu(dy, dtype)), tm(z), tm(P)
    carry = np.zeros((B, Hd), npdt) if dhT is None else _cpu(dhT, dtype).numpy().copy()
    dh_t = np.empty((T, B, Hd), npdt)
    for t in range(T - 1, -1, -1):
        dh_t[t] = dy_t[t] + carry
        carry = dh_t[t] * z_t[t] + P_t[t]
    dh = torch.from_numpy(np.ascontiguousarray(dh_t.transpose(1, 0, 2)))
    a, b = dh * f_r, dh * f_z
    return torch.cat((a, b, dh * f_n), -1), torch.cat((a, b, dh * f_hn), -1), torch.from_numpy(carry)


# ---- which kernel a batch row reaches ------------------------------------------------------------------------------
K_UNITS, MAX_ROWS, MAX_ROWS_BWD, MFMA_ROWS = 16, 64, 16, 16        # kUnits, kMaxRows, kMaxRowsBwd, kMfmaRows
Slice = namedtuple("Slice", "rows BL NG last mfma KP NW RT NRS kernel")


def resident_slots(cus: int, NW: int, spread: bool) -> int:
    slots = cus // NW
    return slots - 1 if spread else slots - slots % 8


def plan(B: int, Hd: int, cus: int, lowp: bool, backward: bool, spread: bool = False, T: int = 1):
    """The launches of a [B, ., Hd] problem on `cus` compute units, as gru.py slices the batch and run_gru plans each slice:
    a list of Slice(rows, BL rows per group, NG groups, rows in the last group, whether a matrix-core kernel runs, KP, NW,
    register tile RT and row sets NRS of an fp32 kernel (0 for a matrix-core one), the instantiation's name).
    The bf16 forward runs a matrix-core kernel only for BL >= 2, the bf16 backward only for T < 65536."""
    if not 0 < Hd <= 512:
        raise ValueError(f"hidden size {Hd}")
    KP = 4 if Hd <= 64 else 8 if Hd <= 128 else 16 if Hd <= 256 else 32
    NW = (Hd + K_UNITS - 1) // K_UNITS
    max_rows = MFMA_ROWS if lowp else (MAX_ROWS_BWD if backward else MAX_ROWS)
    if resident_slots(cus, NW, False) < 8:
        raise ValueError("does not fit")
    cap = (resident_slots(cus, NW, False) - 1) * max_rows            # ddsp_gru_max_batch: the default placement's, in both modes
    slots = resident_slots(cus, NW, spread)
    if slots < (1 if spread else 8):
        raise ValueError("does not fit")
    out = []
    for lo in range(0, B, cap):
        rows = min(B, lo + cap) - lo
        NG = min(rows, slots)
        BL = -(-rows // NG)
        NG = -(-rows // BL)
        if BL > max_rows:
            raise ValueError(f"{BL} rows per group")
        mfma = bool(lowp) and (T < 65536 if backward else BL >= 2)
        if mfma:
            RT = NRS = 0
            kernel = f"gru_{'bwd' if backward else 'fwd'}_mfma_kernel<{KP}>"
        else:
            RT = 4 if backward and 2 < BL <= 4 else 2
            NRS = 1 if BL <= 2 or RT == 4 else 2
            kernel = f"gru_{'bwd' if backward else 'fwd'}_kernel<{KP},{RT},{NRS}>"
        out.append(Slice(rows, BL, NG, rows - (NG - 1) * BL, mfma, KP, NW, RT, NRS, kernel))
    return out


def rounded_rows(slices):
    """One flag per batch row: does the row's slice run a matrix-core kernel (bf16 products)?"""
    return torch.cat([torch.full((s.rows,), s.mfma) for s in slices])


# ---- inputs and the criterion (host test, GPU tests, fuzz sweep) -----------------------------------------------------
def make_inputs(B: int, T: int, Hd: int, seed: int, h0: bool = True, bias: bool = True, dhT: bool = True):
    """W_hh, b_hh uniform +-1/sqrt(Hd) (nn.GRU's initialisation); gi, dy, dhT N(0,1); h0 = tanh(N(0,1)).  With B >= 3, row 0 has
    gi scaled by 8 (saturated gates, factors near 0) and row 1 has gi = 0 and a zero h0.  CPU fp32 tensors (or None)."""
    g = torch.Generator().manual_seed(seed)
    k = 1.0 / math.sqrt(Hd)
    x = dict(gi=torch.randn((B, T, 3 * Hd), generator=g),
             w=(torch.rand((3 * Hd, Hd), generator=g) * 2.0 - 1.0) * k,
             b=(torch.rand((3 * Hd,), generator=g) * 2.0 - 1.0) * k,
             h0=torch.randn((B, Hd), generator=g).tanh(),
             dy=torch.randn((B, T, Hd), generator=g),
             dhT=torch.randn((B, Hd), generator=g))
    if B >= 3:
        x["gi"][0] *= 8.0
        x["gi"][1] = 0.0
        x["h0"][1] = 0.0
    if not h0:
        x["h0"] = None
    if not bias:
        x["b"] = None
    if not dhT:
        x["dhT"] = None
    return x


ABSOLUTE = ("y", "hT", "r", "z", "n")              # live in [-1, 1]: absolute error
RELATIVE = ("hn", "d_gi", "d_gh", "dh0")           # error relative to the reference tensor's largest entry
Measure = namedtuple("Measure", "err e32 gap")


def _measure(got, ref, ref32, other, relative: bool):
    ref = ref.double()
    scale = float(ref.abs().max()) if relative else 1.0
    scale = scale if scale > 0.0 else 1.0
    dist = lambda a: float((a.detach().cpu().double() - ref).abs().max()) / scale if a.numel() else 0.0     # noqa: E731
    return Measure(dist(got), dist(ref32), dist(other))


def _named_forward(h, r, z, n, ghn):
    return {"y": h, "hT": h[:, -1], "r": r, "z": z, "n": n, "hn": ghn}


def forward_measures(x, y, hT, gates, hn, rounded):
    """The kernel's forward outputs against the fp64 reference: {tensor: Measure(err, e32, gap)}.  err: the kernel's distance from
    the fp64 reference; e32: the fp32 reference's; gap: the distance of the fp64 reference with the OTHER rounding.  `gates`, `hn`
    may be None (an inference launch)."""
    B, T, Hd = y.shape
    rows = _rows(rounded, B)
    args = (x["gi"], x["w"], x["b"], x["h0"], y)
    ref = _named_forward(*forward_steps(*args, torch.float64, rows))
    ref32 = _named_forward(*forward_steps(*args, torch.float32, rows))
    other = _named_forward(*forward_steps(*args, torch.float64, ~rows))
    got = {"y": y, "hT": hT}
    if gates is not None:
        g = gates.detach().cpu()
        got.update(r=g[..., :Hd], z=g[..., Hd:2 * Hd], n=g[..., 2 * Hd:], hn=hn)
    return {k: _measure(v, ref[k], ref32[k], other[k], k in RELATIVE) for k, v in got.items()}


def backward_measures(x, y, gates, hn, d_gi, d_gh, dh0, rounded):
    """The kernel's backward outputs (fp32) against the fp64 reference teacher-forced from its `d_gh`: {tensor: Measure}."""
    rows = _rows(rounded, y.shape[0])
    args = (x["dy"], x["dhT"], x["w"], x["h0"], y, gates, hn, d_gh)
    names = ("d_gi", "d_gh", "dh0")
    ref = dict(zip(names, backward_steps(*args, torch.float64, rows)))
    ref32 = dict(zip(names, backward_steps(*args, torch.float32, rows)))
    other = dict(zip(names, backward_steps(*args, torch.float64, ~rows)))
    got = dict(zip(names, (d_gi, d_gh, dh0)))
    return {k: _measure(got[k], ref[k], ref32[k], other[k], True) for k in names}


def failures(measures, T: int, margin: float = MARGIN):
    """The criterion: every tensor within `margin` x e32 of the fp64 reference, where e32 is the distance of the SAME formulas
    evaluated in fp32 on the same inputs, in the same norm.  The margin of 8 covers the two differences between the kernels and
    the fp32 reference: sigmoid / tanh built from the hardware exp2 and rcp (1 ulp each, composed three deep), and another order of
    summation.  Not vacuous: `margin` x e32 has to be at most 1/32 of the distance between the bf16-rounded and the unrounded
    reference on the same inputs -- a case that violates this is reported as a failure of the CASE.  (At T = 1 the backward's
    d_gi / d_gh consume no product, so the two roundings agree on them by construction: only dh0 carries the condition there.)
    -> list of messages, empty when the case passes."""
    bad = []
    for k, m in measures.items():
        if not m.err <= margin * m.e32:
            bad.append(f"{k}: error {m.err:.3e} > {margin:g} x e32 {m.e32:.3e}")
        if T == 1 and k in ("d_gi", "d_gh"):
            continue
        if not margin * m.e32 <= m.gap / GAP_FACTOR:
            bad.append(f"{k}: vacuous case, {margin:g} x e32 {m.e32:.3e} > 1/{GAP_FACTOR:g} of the roundings' distance {m.gap:.3e}")
    return bad


def worst_ratio(measures) -> float:
    """Largest err / e32 over the tensors (an exact match is 0 even against a zero yardstick)."""
    out = 0.0
    for m in measures.values():
        out = max(out, 0.0 if m.err == 0.0 else (m.err / m.e32 if m.e32 > 0.0 else math.inf))
    return out


def describe(measures) -> str:
    return ", ".join(f"{k} {m.err:.1e}/{m.e32:.1e} (gap {m.gap:.1e})" for k, m in measures.items())


def bf16_ulp(ref):
    """One bf16 ulp at the magnitude of each entry of `ref` (fp64): 2^(exponent - 7)."""
    _, e = torch.frexp(ref.double().abs().clamp_min(2.0 ** -126))      # |ref| = m 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(ref, dtype=torch.float64), e - 8)
