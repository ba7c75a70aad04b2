"""Host test of the invariant the chunked oscillator's walks compile in (csrc/ddsp_osc_plan.h: derived_shift).

A derived slot's phase is 2^t times its root's.  The kernels take t from `derived_shift(K, d)` at compile time instead of
reading `PlanTable::shift` per lane, which is only right if the planner gives every FILLED derived slot d exactly that shift, in
every lane of every plan.  For every K that has derived slots x G in {4, 8, 16} x H = 1..400 that `plan_slots` accepts:
`shift == derived_shift(K, d)`, and the parent's harmonic number times 2^shift is the slot's own.  Padded derived slots
(amplitude 0) are counted, not checked: they carry shift 0 in the table and the kernels keep them out of their range tests.

The plan header is plain C++; the test compiles tests/osc_plan_shift_check.cpp against it, as test_osc_slot_plan_host.py does
with its dump program -- which is also where the list of K comes from (its first line).
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HMAX = 400
# slot_children per K, written out again here: derived slots are numbered root slot by root slot, child r of a root has t = r + 1
CHILDREN = {4: (1,), 8: (2, 1), 12: (3, 2, 1), 13: (3, 2, 1), 15: (3, 2, 1, 1), 16: (3, 2, 1, 1), 20: (3, 2, 2, 1, 1),
            23: (3, 2, 2, 1, 1, 1), 25: (3, 2, 2, 1, 1, 1, 1)}


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None and os.path.exists("/opt/rocm/llvm/bin/clang++"):
        cxx = "/opt/rocm/llvm/bin/clang++"
    assert cxx, "a host C++ compiler is needed to read the slot plans"
    tmp = tmp_path_factory.mktemp("shift")
    exe, dump = str(tmp / "osc_plan_shift_check"), str(tmp / "osc_slot_plan_dump")
    for out, opt in ((exe, "-O2"), (dump, "-O0")):
        subprocess.run([cxx, "-std=c++17", opt, "-I", os.path.join(ROOT, "ddsp-pytorch_amd", "csrc"),
                        os.path.join(ROOT, "tests", os.path.basename(out) + ".cpp"), "-o", out], check=True)
    first = subprocess.run([dump], check=True, capture_output=True, text=True).stdout.split()
    assert first[0] == "ks"
    KS = tuple(int(v) for v in first[1:])
    # (one process per K, side by side: the planner's search over 1 200 shapes per K is what takes the time)
    procs = [subprocess.Popen([exe, str(HMAX), str(k)], stdout=subprocess.PIPE, text=True) for k in KS]
    txt = []
    for pr in procs:
        out, _ = pr.communicate()
        assert pr.returncode == 0
        txt += out.splitlines()
    per_k, shifts, bad = {}, {}, []
    for line in txt:
        w = line.split()
        if w[0] == "K":
            per_k[int(w[1])] = {w[i]: int(w[i + 1]) for i in range(2, len(w), 2)}
        elif w[0] == "shifts":
            shifts[int(w[1])] = [int(v) for v in w[3:]]
        else:
            bad.append(line)
    return per_k, shifts, bad, KS


def test_every_filled_derived_slot_has_the_compile_time_shift(report):
    per_k, _, bad, KS = report
    assert sorted(per_k) == sorted(KS)
    assert not bad, bad[:10]
    for K in KS:
        r = per_k[K]
        assert r["violations"] == 0, (K, r)
        assert r["plans"] > 0 and r["filled"] > 0, (K, r)       # ... and the loop was not empty
    assert sum(r["plans"] for r in per_k.values()) > 1000
    assert sum(r["padded"] for r in per_k.values()) > 0          # padded derived slots exist: the kernels' mask has a reader


def test_derived_shift_is_rank_plus_one(report):
    _, shifts, _, KS = report
    assert sorted(KS) == sorted(CHILDREN)
    for K in KS:
        want = [r + 1 for n in CHILDREN[K] for r in range(n)]
        assert shifts[K] == want, (K, shifts[K], want)
    assert sorted(set(shifts[13])) == [1, 2, 3]                  # three factors at the benchmark's K
