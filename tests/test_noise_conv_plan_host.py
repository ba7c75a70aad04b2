"""Host test of the index plan of the hop-128 noise convolution on the matrix cores (csrc/ddsp_noise_conv_plan.h): which (tap, source)
pairs the 576 instructions of a group multiply, which outputs they add to, and which LDS floats they read.

The plan header is plain C++; the test compiles tests/noise_conv_plan_dump.cpp against it and reads the plan as text.  An instruction
(mu, a, beta) gives, for i, j in 0..3, the product k[tap_base + i] * x[src_base + 4 j] to output 16 window + i + 4 j of every frame."""
import collections
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 128


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None and os.path.exists("/opt/rocm/llvm/bin/clang++"):
        cxx = "/opt/rocm/llvm/bin/clang++"
    assert cxx, "a host C++ compiler is needed to read the convolution plan"
    exe = str(tmp_path_factory.mktemp("plan") / "noise_conv_plan_dump")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "ddsp-pytorch_amd", "csrc"),
                    os.path.join(ROOT, "tests", "noise_conv_plan_dump.cpp"), "-o", exe], check=True)
    dims, steps, tap_slot, src_slot = None, [], {}, {}
    for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines():
        w = line.split()
        if w[0] == "dims":
            keys = ("frames", "samples", "steps", "tap_pad", "tap_stride", "tap_floats", "src_pad", "src_row", "src_plane", "src_floats")
            dims = dict(zip(keys, map(int, w[1:])))
        elif w[0] == "step":
            keys = ("mu", "a", "beta", "window", "tap_base", "src_base", "tap_offset", "src_offset")
            steps.append(dict(zip(keys, map(int, w[1:]))))
        else:
            (tap_slot if w[1] == "tap" else src_slot)[(int(w[2]), int(w[3]))] = int(w[4])
    return dims, steps, tap_slot, src_slot


def test_every_pair_of_the_truncated_convolution_exactly_once(plan):
    dims, steps, _, _ = plan
    assert (dims["frames"], dims["samples"]) == (16, N)
    assert len(steps) == dims["steps"] == 576 and len({(s["mu"], s["a"], s["beta"]) for s in steps}) == 576
    seen = collections.Counter()
    padded = 0
    for s in steps:
        assert s["tap_base"] == 16 * s["a"] + s["mu"] and s["src_base"] == 16 * s["beta"] - s["mu"] and s["window"] == s["a"] + s["beta"]
        assert 0 <= s["window"] < 8
        for i in range(4):
            for j in range(4):
                m, p = s["tap_base"] + i, s["src_base"] + 4 * j
                assert m + p == 16 * s["window"] + i + 4 * j            # the output the instruction adds this product to
                if m >= 0 and p >= 0:
                    seen[(m, p)] += 1
                else:
                    padded += 1                                         # reads padding: m < 0 or p < 0
    want = {(m, p) for m in range(N) for p in range(N) if m + p < N}
    assert set(seen) == want and set(seen.values()) == {1}              # m + p < 128 follows from the window; none is missing or double
    assert len(want) == 8256 and padded == 576 * 16 - 8256


def test_every_read_stays_inside_the_padded_rows_and_pairs_with_its_slot(plan):
    dims, steps, tap_slot, src_slot = plan
    assert dims["tap_floats"] == 16 * dims["tap_stride"] and dims["src_floats"] == 4 * dims["src_plane"] == 4 * 16 * dims["src_row"]
    assert len(set(tap_slot.values())) == len(tap_slot) == dims["tap_floats"]         # the slots tile the two tiles exactly
    assert len(set(src_slot.values())) == len(src_slot) == dims["src_floats"]
    assert set(tap_slot.values()) == set(range(dims["tap_floats"])) and set(src_slot.values()) == set(range(dims["src_floats"]))
    for s in steps:
        for b in range(16):
            for q in range(4):
                # the float lane 4 b + q reads is the slot of the tap / the sample the plan says it multiplies
                assert s["tap_offset"] + b * dims["tap_stride"] + q == tap_slot[(b, s["tap_base"] + q)]
                assert s["src_offset"] + b * dims["src_row"] + q == src_slot[(b, s["src_base"] + 4 * q)]
    assert min(s["tap_base"] for s in steps) == -3 >= -dims["tap_pad"] and min(s["src_base"] for s in steps) == -12 >= -dims["src_pad"]
    assert max(s["tap_base"] for s in steps) + 3 == N - 1 and max(s["src_base"] for s in steps) + 12 == N - 1


def test_operand_reads_are_bank_conflict_free(plan):
    """A ds_read_b32 serves lanes 0..31, then lanes 32..63; the bank is the dword address modulo 32.  The compiler emits the reads in
    pairs as ds_read2_b32, which is served as two ds_read_b32, one per dword: each dword of a pair is one of the reads enumerated here."""
    dims, steps, _, _ = plan
    for s in steps:
        for half in range(2):
            lanes = range(32 * half, 32 * half + 32)
            a_banks = {(s["tap_offset"] + (ln >> 2) * dims["tap_stride"] + (ln & 3)) % 32 for ln in lanes}
            b_banks = {(dims["tap_floats"] + s["src_offset"] + (ln >> 2) * dims["src_row"] + (ln & 3)) % 32 for ln in lanes}
            assert len(a_banks) == 32 and len(b_banks) == 32

