"""Host tests of the chunked oscillator's slot plan (csrc/ddsp_osc_plan.h) and of the identity it rests on.

The identity: in the reference, the per-sample increment and the unwrapped fp32 phase of harmonic 2m are bit for bit twice those
of harmonic m (a factor of two commutes with every rounding between f0 and the phase).  Checked on the
reference's own recorded `inc` / `cum` (fixtures g1, g5, g6) and on the oracle's restatement for random, zero, negative, NaN and
tiny f0; the control -- harmonic 3 against three times harmonic 1 -- must NOT hold, or the comparison would be blind.

The planner: every (H, K, G) the tilings can hand to the chunked form, plus H = 1, 2, 3.  The plan header is plain C++; the
test compiles tests/osc_slot_plan_dump.cpp against it and reads the plans as text.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def assert_doubling(arr, what):
    """arr [..., H]: column of harmonic 2m == 2 * column of harmonic m, bit for bit (NaN matches NaN)."""
    H = arr.shape[-1]
    n = 0
    for m in range(1, H // 2 + 1):
        lo, hi = arr[..., m - 1], arr[..., 2 * m - 1]
        with np.errstate(over="ignore", invalid="ignore"):
            twice = (lo * np.float32(2.0)).astype(np.float32)
        same = (bits(twice) == bits(hi)) | (np.isnan(twice) & np.isnan(hi))
        assert same.all(), f"{what}: harmonic {2 * m} != 2 * harmonic {m} in {int((~same).sum())} of {same.size} values"
        n += same.size
    return n


@pytest.mark.parametrize("name", ["g1_osc_tiny", "g5_osc_nyquist", "g6_osc_hop100", "g6_osc_hop160", "g6_osc_hop3", "g6_osc_hop441",
                                  "g6_osc_hop480", "g6_osc_hop7", "g6_osc_single_frame"])
def test_even_harmonics_double_in_the_reference_fixtures(golden, name):
    g = golden(name)
    assert assert_doubling(g["inc"], name + " inc") > 0
    assert assert_doubling(g["cum"], name + " cum") > 0


@pytest.mark.parametrize("kind", ["random", "zero", "negative", "nan", "tiny"])
@pytest.mark.parametrize("H,hop,sr", [(100, 128, 16000), (60, 100, 16000), (200, 512, 48000)])
def test_even_harmonics_double_in_the_oracle(kind, H, hop, sr):
    rng = np.random.default_rng(17)
    B, T = 3, 9
    f0 = rng.uniform(20.0, 2000.0, (B, T, 1)).astype(np.float32)
    if kind == "zero":
        f0[1] = 0.0
        f0[2, 3:5] = 0.0
    elif kind == "negative":
        f0[1] = -50.0
        f0[2, 4] = -220.0
    elif kind == "nan":
        f0[1, 2] = np.nan
        f0[2, 6] = np.inf
    elif kind == "tiny":
        f0[1] = 1e-30
        f0[2, 2:4] = 1e-30
    c = rng.uniform(0.1, 1.0, (B, T, H)).astype(np.float32)
    a = rng.uniform(0.1, 1.0, (B, T, 1)).astype(np.float32)
    _, dbg = oracle.osc_forward(f0, c, a, hop, sr, debug=True)
    assert_doubling(dbg["inc"], "inc")
    assert_doubling(dbg["cum"], "cum")
    if kind == "random":    # the control: a factor of three does not commute with the roundings
        with np.errstate(over="ignore", invalid="ignore"):
            thrice = (dbg["cum"][..., 0] * np.float32(3.0)).astype(np.float32)
        assert (bits(thrice) != bits(dbg["cum"][..., 2])).mean() > 0.05


# ---- the planner ------------------------------------------------------------------------------------------------------
def selectable(ks):
    """(H, K, G) the chunked form can be launched with: pick_tiling's G for every K, 4..16 lanes per row."""
    out = []
    for K in ks:
        for H in range(1, 401):
            lanes = -(-H // K)
            G = 1
            while G < lanes:
                G *= 2
            if G in (4, 8, 16):
                out.append((H, K, G))
    return out


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None and os.path.exists("/opt/rocm/llvm/bin/clang++"):
        cxx = "/opt/rocm/llvm/bin/clang++"
    assert cxx, "a host C++ compiler is needed to read the slot plans"
    exe = str(tmp_path_factory.mktemp("plan") / "osc_slot_plan_dump")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "ddsp-pytorch_amd", "csrc"),
                    os.path.join(ROOT, "tests", "osc_slot_plan_dump.cpp"), "-o", exe], check=True)

    def get(triples):
        res = {}
        for i in range(0, len(triples), 200):
            args = [str(v) for t in triples[i:i + 200] for v in t]
            txt = subprocess.run([exe] + args, check=True, capture_output=True, text=True).stdout.splitlines()
            cur = None
            for line in txt:
                w = line.split()
                if w[0] == "ks":
                    continue
                if w[0] == "plan":
                    H, K, G, ok, KR, KD = (int(v) for v in w[1:7])
                    cur = dict(H=H, K=K, G=G, ok=ok, KR=KR, KD=KD, cls=[int(v) for v in w[7:11]], lanes=[], parents=[])
                    res[(H, K, G)] = cur
                elif w[0] == "parents":
                    cur["parents"] = [int(v) for v in w[3:]]
                else:
                    cur["lanes"].append([tuple(int(v) for v in s.split("/")) for s in w[3:]])
        return res
    first = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    assert first[0] == "ks"
    get.ks = tuple(int(v) for v in first[1:])           # the list of K (csrc/ddsp_osc_plan.h: DDSP_OSC_KS)
    return get


def check_plan(p):
    H, K, G, KR, KD = p["H"], p["K"], p["G"], p["KR"], p["KD"]
    assert KR + KD == K and len(p["lanes"]) == G and all(len(l) == K for l in p["lanes"])      # loop bounds uniform over lanes
    seen = sorted(h for lane in p["lanes"] for h, _ in lane if h)
    assert seen == list(range(1, H + 1)), "every harmonic in exactly one slot"
    if not p["ok"]:
        assert KD == 0
        for j, lane in enumerate(p["lanes"]):
            for m, (h, t) in enumerate(lane):
                assert h == (j + m * G + 1 if j + m * G < H else 0) and t == 0      # today's mapping
    else:
        assert KD >= 1 and KR * G <= H and len(p["parents"]) == KD
        assert any(h for lane in p["lanes"] for h, _ in lane[KR:])
        for lane in p["lanes"]:
            for m, (h, t) in enumerate(lane):
                if m < KR:
                    assert t == 0
                elif h:                                         # a derived slot: its parent is a root slot of the same lane
                    parent = lane[p["parents"][m - KR]][0]
                    assert parent and t >= 1 and h == parent << t
    # class limits: every harmonic up to cls[q] sits inside class q's prefixes (of the roots, and of the derived slots they feed)
    frac = [lambda n: (3 * n + 3) // 4, lambda n: (n + 1) // 2, lambda n: (n + 3) // 4, lambda n: (n + 7) // 8]
    for q in range(4):
        nr = frac[q](KR)
        nd = sum(1 for par in p["parents"] if par < nr)
        assert p["parents"][:nd] == [par for par in p["parents"] if par < nr]       # ... which are a prefix
        for lane in p["lanes"]:
            for m, (h, _) in enumerate(lane):
                inside = m < nr if m < KR else (m - KR) < nd
                assert inside or h == 0 or h > p["cls"][q]
        assert 0 <= p["cls"][q] <= H
    assert p["cls"] == sorted(p["cls"], reverse=True)


def test_the_list_of_k(plans):
    assert plans.ks == (4, 8, 12, 13, 15, 16, 20, 23, 25)


def test_planner_properties_for_every_selectable_shape(plans):
    triples = selectable(plans.ks)
    got = plans(triples)
    assert len(got) == len(triples) > 1000
    for t in triples:
        check_plan(got[t])


def test_shipped_shapes_get_derived_slots(plans):
    # (H, K, G) of the benchmark's and the tests' shapes: the split the kernels are instantiated for
    want = {(100, 13, 8): (7, 6), (200, 13, 16): (7, 6), (60, 15, 4): (8, 7), (180, 12, 16): (6, 6), (64, 16, 4): (9, 7),
            (100, 25, 4): (14, 11)}
    got = plans(list(want))
    for t, (KR, KD) in want.items():
        assert got[t]["ok"] == 1 and (got[t]["KR"], got[t]["KD"]) == (KR, KD), (t, got[t]["KR"], got[t]["KD"])
        check_plan(got[t])


def test_fallback_where_no_packing_exists(plans):
    # H = 1, 2, 3 (no room for a root column per slot), and 50 harmonics on 4 lanes of 13 (the 7 + 6 shape does not pack)
    triples = [(1, 4, 4), (2, 4, 4), (3, 4, 4), (50, 13, 4)]
    got = plans(triples)
    for t in triples:
        assert got[t]["ok"] == 0 and got[t]["KD"] == 0 and got[t]["KR"] == t[1]
        check_plan(got[t])
