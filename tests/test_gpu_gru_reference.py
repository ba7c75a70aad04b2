"""The GRU recurrence's kernels (csrc/ddsp_gru.hip), fp32 and bf16 matrix-core, against the fp64 reference of tests/gru_reference.py:
one step at a time from the kernel's own previous output, so that the bf16 kernels' per-step rounding cannot fall differently in the
reference, and the bound is fp32 round-off -- every tensor within 8 x e32, e32 being the same formulas evaluated in fp32
(gru_reference.failures; tests/test_gru_reference_host.py shows that seven seeded bugs of the bf16 kernels sit 100 x above it).
Every case states through gru_reference.plan which instantiation and which rounding its rows reach, on the 256 CUs of an MI355X.

Measured on an MI355X, the worst error / e32 (bound: 8) over the cases of this module | over seed 707 of fuzz_parity.sweep_gru:
    fp32 forward   1.70 | 2.88        bf16 forward   2.93 | 2.46
    fp32 backward  1.69 | 1.76        bf16 backward  2.60 | 2.14
e32 itself is 0.5e-7 .. 4e-7 (absolute on y / hT / r / z / n, of the largest entry on hn and the gradients), the two roundings lie
2e-4 .. 3e-3 apart.  No kernel or launcher bug showed: the margin of 8 stands as set.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import fuzz_parity  # noqa: E402
import gru_reference as R  # noqa: E402

CUS = 256


def _run(B, T, Hd, lowp, seed, **kw):
    assert torch.cuda.get_device_properties(0).multi_processor_count == CUS      # the plans below are stated for an MI355X
    r = fuzz_parity.gru_case(B, T, Hd, lowp, seed, **kw)
    print(f"B{B} T{T} Hd{Hd} lowp {int(lowp)} {kw}: {fuzz_parity.gru_case_line(r)}")
    return r


def _kernels(r):
    return [s.kernel for s in r["plan_fwd"]], [s.kernel for s in r["plan_bwd"]]


# (B, Hd) of the table in tests/test_gru.py -> rows per group, and the fp32 instantiations they reach: <RT,NRS> forward, backward
_INSTANTIATIONS = [
    (70, 64, 2, "2,1", "2,1"), (200, 64, 4, "2,2", "4,1"), (330, 64, 6, "2,2", "2,2"),
    (40, 100, 2, "2,1", "2,1"), (100, 100, 4, "2,2", "4,1"), (160, 100, 5, "2,2", "2,2"),
    (20, 200, 2, "2,1", "2,1"), (50, 200, 4, "2,2", "4,1"), (80, 200, 5, "2,2", "2,2"),
    (12, 512, 2, "2,1", "2,1"), (32, 512, 4, "2,2", "4,1"), (40, 512, 5, "2,2", "2,2"),
]


def _expected(B, Hd, lowp, fwd, bwd):
    KP = {64: 4, 100: 8, 200: 16, 512: 32}[Hd]
    if lowp:
        return [f"gru_fwd_mfma_kernel<{KP}>"], [f"gru_bwd_mfma_kernel<{KP}>"]
    return [f"gru_fwd_kernel<{KP},{fwd}>"], [f"gru_bwd_kernel<{KP},{bwd}>"]


def test_the_pinned_cases_reach_all_28_instantiations():
    reached = set()
    for B, Hd, BL, fwd, bwd in _INSTANTIATIONS:
        for lowp in (False, True):
            f, b = _expected(B, Hd, lowp, fwd, bwd)
            assert [s.kernel for s in R.plan(B, Hd, CUS, lowp, False)] == f and [s.kernel for s in R.plan(B, Hd, CUS, lowp, True)] == b
            reached.update(f + b)
    want = {f"gru_fwd_kernel<{KP},{v}>" for KP in (4, 8, 16, 32) for v in ("2,1", "2,2")}
    want |= {f"gru_bwd_kernel<{KP},{v}>" for KP in (4, 8, 16, 32) for v in ("2,1", "4,1", "2,2")}
    want |= {f"gru_{d}_mfma_kernel<{KP}>" for KP in (4, 8, 16, 32) for d in ("fwd", "bwd")}
    assert len(want) == 28 and reached == want


@pytest.mark.parametrize("lowp", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,Hd,BL,fwd,bwd", _INSTANTIATIONS)
def test_every_instantiation_matches_fp64_step_by_step(B, Hd, BL, fwd, bwd, lowp):
    T = 5 + (B + Hd) % 4                                  # 5 .. 8
    r = _run(B, T, Hd, lowp, 1000 + B + Hd, h0=bool(B % 4 == 0))
    assert _kernels(r) == _expected(B, Hd, lowp, fwd, bwd)
    assert [s.BL for s in r["plan_fwd"]] == [BL] and [s.BL for s in r["plan_bwd"]] == [BL]
    assert not r["bad"], r["bad"]


# hidden sizes: not a multiple of 8 (partial 8-vectors in the fragments: 12, 33, 100, 250, 257, 500), not a multiple of 16 (a partial
# last workgroup: 12, 33, 100, 200, 250, 257, 500), exactly HP (64, 512), one past a KP boundary (257); B gives 2 rows per group
@pytest.mark.parametrize("lowp", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("Hd,B,KP", [(12, 300, 4), (33, 100, 4), (64, 70, 4), (100, 40, 8), (200, 20, 16), (250, 20, 16), (257, 12, 32),
                                     (500, 12, 32), (512, 12, 32)])
def test_hidden_sizes_and_masks(Hd, B, KP, lowp):
    r = _run(B, 5, Hd, lowp, 2000 + Hd)
    for s in r["plan_fwd"] + r["plan_bwd"]:
        assert (s.KP, s.BL, s.mfma) == (KP, 2, lowp), s
    assert not r["bad"], r["bad"]


# rows per group of the bf16 kernels: (B, Hd) -> (BL, groups, rows in the last group)
@pytest.mark.parametrize("with_h0", [True, False], ids=["h0", "no-h0"])
@pytest.mark.parametrize("B,Hd,BL,NG,last", [
    (16, 512, 2, 8, 2),           # BL = 2
    (24, 512, 3, 8, 3),           # odd BL: the forward packs rows in pairs, the odd row's neighbour is past the last row
    (20, 512, 3, 7, 2),           # a shorter last group
    (9, 512, 2, 5, 1),            # exactly one row in the last group of BL = 2
    (36, 512, 5, 8, 1),           # ... and of an odd BL = 5
    (112, 512, 14, 8, 14),        # the largest BL at 512 units
    (1008, 64, 16, 63, 16),       # the largest BL there is: every row of the MFMA tile
    (1000, 64, 16, 63, 8),        # ... with a half-filled last group
])
def test_rows_per_group_of_the_bf16_kernels(B, Hd, BL, NG, last, with_h0):
    r = _run(B, 3 + B % 3, Hd, True, 3000 + B, h0=with_h0)
    for s in r["plan_fwd"] + r["plan_bwd"]:
        assert (s.rows, s.BL, s.NG, s.last, s.mfma) == (B, BL, NG, last, True), s
    assert not r["bad"], r["bad"]


@pytest.mark.parametrize("with_h0", [True, False], ids=["h0", "no-h0"])
def test_one_row_per_group_takes_the_fp32_forward_and_the_bf16_backward(with_h0):
    r = _run(6, 4, 512, True, 3100, h0=with_h0)
    assert _kernels(r) == (["gru_fwd_kernel<32,2,1>"], ["gru_bwd_mfma_kernel<32>"])
    assert r["plan_bwd"][0].BL == 1
    assert not r["bad"], r["bad"]


# T = 1 keeps h0: without it W_hh meets zeros only and no rounding could be told apart (gru_reference.failures' condition)
@pytest.mark.parametrize("lowp", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("T,with_h0", [(1, True), (2, True), (2, False), (3, False), (4, True)])
def test_short_sequences(T, with_h0, lowp):
    r = _run(40, T, 100, lowp, 4000 + T, h0=with_h0)
    assert _kernels(r) == _expected(40, 100, lowp, "2,1", "2,1")
    assert not r["bad"], r["bad"]


@pytest.mark.parametrize("lowp", [False, True], ids=["fp32", "bf16"])
def test_without_bias_and_without_dhT(lowp):
    r = _run(50, 6, 200, lowp, 5000, bias=False, dhT=False)
    assert _kernels(r) == _expected(50, 200, lowp, "2,2", "4,1")
    assert not r["bad"], r["bad"]


def test_a_one_row_tail_slice_runs_the_fp32_forward_next_to_the_bf16_one():
    r = _run(113, 3, 512, True, 6000)
    assert [(s.rows, s.BL, s.kernel) for s in r["plan_fwd"]] == [(112, 14, "gru_fwd_mfma_kernel<32>"), (1, 1, "gru_fwd_kernel<32,2,1>")]
    assert [(s.rows, s.BL, s.kernel) for s in r["plan_bwd"]] == [(112, 14, "gru_bwd_mfma_kernel<32>"), (1, 1, "gru_bwd_mfma_kernel<32>")]
    assert R.rounded_rows(r["plan_fwd"]).tolist() == [True] * 112 + [False]          # row 112 is held to the UNROUNDED reference
    assert not r["bad"], r["bad"]


def test_the_last_16_bit_epoch_of_the_bf16_backward():
    r = _run(2, 65535, 12, True, 7000)
    assert _kernels(r) == (["gru_fwd_kernel<4,2,1>"], ["gru_bwd_mfma_kernel<4>"])
    assert not r["bad"], r["bad"]


@pytest.mark.parametrize("io16", [False, True], ids=["fp32-out", "io16"])
def test_65536_steps_take_the_fp32_backward(io16):
    """With io16 the bf16 entry point refuses (the fp32 kernels write fp32 only) and gru.py redoes the slice with fp32 outputs and
    casts them: gru_case checks that the 16-bit tensors are the bf16 cast of the fp32 launch's and dh0 is bitwise the same."""
    r = _run(2, 65536, 12, True, 7001, io16=io16)
    assert _kernels(r) == (["gru_fwd_kernel<4,2,1>"], ["gru_bwd_kernel<4,2,1>"])
    assert R.rounded_rows(r["plan_bwd"]).tolist() == [False, False]
    assert not r["bad"], r["bad"]


@pytest.mark.parametrize("B,Hd,BL,NG", [(14, 512, 2, 7), (40, 200, 3, 14)])
def test_bf16_kernels_in_the_spread_placement(B, Hd, BL, NG):
    """ddsp_gru_set_mode(1) deals every group's workgroups over all XCDs: both bf16 kernels meet the criterion there, and are
    bitwise equal to the default placement -- a row's sums do not depend on its slot in the group."""
    base = _run(B, 7, Hd, True, 8000 + B, keep=True)
    got = _run(B, 7, Hd, True, 8000 + B, spread=True, keep=True)
    for r in (base, got):
        assert all(s.mfma and s.BL >= 2 for s in r["plan_fwd"] + r["plan_bwd"])
        assert not r["bad"], r["bad"]
    assert [(s.BL, s.NG) for s in got["plan_fwd"] + got["plan_bwd"]] == [(BL, NG)] * 2
    for a, c in zip(base["out"], got["out"]):
        assert torch.equal(a, c)
