"""Host tests of the filtered-noise planner (csrc/ddsp_noise_plan.h): which kernel form ddsp_noise_forward_ws and
ddsp_noise_backward_ws take for a shape, a mode of ddsp_noise_set_generic and what the host knows of the pointers.

The plan header is plain C++; the test compiles tests/noise_plan_dump.cpp against it and reads the plans as text.  The backward's
plans are held against fuzz_parity.noise_bwd_form, the Python statement of the same dispatch that the form assertions of
test_gpu_noise_backward.py rest on; the forward's against expectations written out here and against fuzz_parity.noise_fwd_form, on
which the form assertions of test_gpu_noise_forward.py rest."""
import os
import shutil
import subprocess

import pytest

import ddsp_pytorch_amd as ddsp
import fuzz_parity as fz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ALIGNED, Y_MISALIGNED, U_ALIGNED, U_MISALIGNED = "11001", "01001", "11111", "11101"     # y, Hmag, u given, u, workspace


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None and os.path.exists("/opt/rocm/llvm/bin/clang++"):
        cxx = "/opt/rocm/llvm/bin/clang++"
    assert cxx, "a host C++ compiler is needed to read the noise plans"
    exe = str(tmp_path_factory.mktemp("plan") / "noise_plan_dump")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "ddsp-pytorch_amd", "csrc"),
                    os.path.join(ROOT, "tests", "noise_plan_dump.cpp"), "-o", exe], check=True)

    def run(queries):
        """queries: (dir, B, T, F, hop, mode, facts, ws) -> one dict per query"""
        out = []
        for i in range(0, len(queries), 500):
            args = [":".join(str(v) for v in q) for q in queries[i:i + 500]]
            for line in subprocess.run([exe] + args, check=True, capture_output=True, text=True).stdout.splitlines():
                w = line.split()
                if w[0] == "ws":
                    out.append(dict(bytes=int(w[5])))
                else:
                    d = dict(kv.split("=") for kv in w[6:])
                    out.append({k: v if k in ("form", "rest") else int(v) for k, v in d.items()})
        assert len(out) == len(queries)
        return out
    return run


# ---- backward -----------------------------------------------------------------------------------------------------------
# every (F, hop) of test_gpu_noise_backward.py, and a few more
BWD_SHAPES = sorted({(257, 512), (194, 512), (195, 512), (223, 512), (224, 512),
                     (2, 8), (9, 16), (65, 8), (33, 40), (65, 128), (64, 128), (129, 64), (65, 160), (128, 256), (129, 256),
                     (101, 512), (200, 480), (1025, 1024),
                     (9, 1), (5, 3), (33, 7), (65, 12), (33, 100), (129, 441), (1025, 2048), (65, 7), (33, 64),
                     (129, 8192)})


def bwd_letter(p):
    assert p["status"] == 0
    if p["form"] == "Fft":
        return "B" if p["ir"] else "A"
    assert p["ir"] == 0
    return {"Batched": f"C{p['lpf']}", "Frame": "D"}[p["form"]]


def test_backward_plan_is_what_the_python_mirror_says(dump):
    cases = [(F, hop, T, mode, facts) for F, hop in BWD_SHAPES for T in (511, 512, 600) for mode in (0, 1, 2, 16)
             for facts in (ALIGNED, Y_MISALIGNED, U_ALIGNED, U_MISALIGNED)]
    with_ws = dump([("b", 1, T, F, hop, mode, facts, "0") for F, hop, T, mode, facts in cases])
    without = dump([("b", 1, T, F, hop, mode, facts, "none") for F, hop, T, mode, facts in cases])
    seen = set()
    for (F, hop, T, mode, facts), pw, pn in zip(cases, with_ws, without):
        aligned = facts in (ALIGNED, U_ALIGNED)
        got = bwd_letter(pw)
        assert got == fz.noise_bwd_form(1, T, F, hop, mode=mode, aligned=aligned), (F, hop, T, mode, facts)
        # no workspace: what mode bit 4 (the cosine sums despite a workspace) plans
        assert bwd_letter(pn) == fz.noise_bwd_form(1, T, F, hop, mode=mode | 16, aligned=aligned), (F, hop, T, mode, facts)
        if mode == 0 and aligned and F == 195:
            assert bwd_letter(pn).startswith("C")
        if mode == 0 and aligned and F == 257:
            assert bwd_letter(pn) == "A"
        if pw["form"] == "Batched":
            assert pw["lpf"] == fz.noise_bwd_lpf_log(F, hop)
        seen.add(got[0])
    assert seen == {"A", "B", "C", "D"}


def test_backward_frame_kernel_out_of_lds(dump):
    (p,) = dump([("b", 1, 3, 2, 32768, 0, ALIGNED, "none")])
    assert p["form"] == "Frame" and p["status"] == -2       # DDSP_ERANGE


# ---- forward ------------------------------------------------------------------------------------------------------------
def fwd(form, ir=0, wave=0, rest="None", lpf=0, status=0):
    return dict(form=form, ir=ir, wave=wave, rest=rest, lpf=lpf, status=status)


FWD_CASES = []      # (B, T, F, hop, mode, facts, ws, expected)
# hop 128 / 65 bands: whole groups of 16 frames to the wavefront form, the rest to the batched kernel (32 frames per workgroup)
for frames, want in ((15, fwd("Batched", lpf=1)), (16, fwd("Wave", wave=16)), (17, fwd("Wave", wave=16, rest="Batched", lpf=1)),
                     (500, fwd("Wave", wave=496, rest="Batched", lpf=1))):
    FWD_CASES.append((1, frames, 65, 128, 0, ALIGNED, "none", want))
    FWD_CASES.append((1, frames, 65, 128, 8, ALIGNED, "none", fwd("Batched", lpf=1)))
    FWD_CASES.append((1, frames, 65, 128, 1, ALIGNED, "none", fwd("Frame")))
FWD_CASES += [(1, 500, 65, 128, 0, "10001", "none", fwd("Batched", lpf=1)),          # Hmag misaligned
              (1, 500, 65, 128, 0, U_MISALIGNED, "none", fwd("Batched", lpf=1)),
              (1, 500, 65, 128, 0, Y_MISALIGNED, "none", fwd("Frame"))]
# hop 512: the FFT form; the product only at its shapes, from 4096 frames, with a whole aligned workspace
for F in (257, 195):
    for frames in (4095, 4096):
        for ws in ("none", "0", "-16"):
            product = F == 195 and frames == 4096 and ws == "0"
            FWD_CASES.append((1, frames, F, 512, 0, ALIGNED, ws, fwd("Fft", ir=int(product))))
        FWD_CASES.append((1, frames, F, 512, 2, ALIGNED, "0", fwd("Batched", lpf=3)))
        FWD_CASES.append((1, frames, F, 512, 16, ALIGNED, "0", fwd("Fft")))
FWD_CASES += [(1, 4096, 195, 512, 0, "11000", "0", fwd("Fft")),                       # workspace misaligned
              (2, 2100, 195, 512, 0, U_ALIGNED, "0", fwd("Fft", ir=1)),
              # y misaligned: the frame kernel, and NO product before it that nothing would read
              (2, 2100, 195, 512, 0, Y_MISALIGNED, "0", fwd("Frame")),
              (2, 2100, 195, 512, 0, U_MISALIGNED, "0", fwd("Batched", lpf=3)),
              (1, 300, 129, 256, 0, ALIGNED, "none", fwd("Batched", lpf=2)),
              (1, 300, 129, 256, 4, ALIGNED, "none", fwd("Fft")),
              (1, 300, 129, 256, 4, Y_MISALIGNED, "none", fwd("Frame")),
              (3, 50, 7, 24, 0, ALIGNED, "none", fwd("Batched")),
              (3, 50, 5, 8, 0, ALIGNED, "none", fwd("Batched")),
              (1, 3, 129, 8192, 0, ALIGNED, "none", fwd("Frame")),                    # no tile of 8 frames fits in LDS
              (1, 3, 8192, 129, 0, ALIGNED, "none", fwd("Frame")),
              (1, 3, 2, 32768, 0, ALIGNED, "none", fwd("Frame", status=-2))]          # nor does one frame: DDSP_ERANGE
for l in range(4):
    FWD_CASES.append((1, 15, 65, 128, (l + 1) << 8, ALIGNED, "none", fwd("Batched", lpf=l)))
    FWD_CASES.append((1, 500, 65, 128, (l + 1) << 8, ALIGNED, "none", fwd("Wave", wave=496, rest="Batched", lpf=l)))


def test_forward_plans(dump):
    got = dump([("f",) + c[:7] for c in FWD_CASES])
    for c, p in zip(FWD_CASES, got):
        p = dict(p)
        lds = p.pop("lds")
        assert p == c[7], (c[:7], p)
        direct = p["form"] in ("Batched", "Frame") or p["rest"] != "None"
        assert (lds > 0) == direct, (c[:7], lds)
        if p["status"] == 0:
            assert lds <= 160 * 1024 or (c[4] >> 8), (c[:7], lds)


def fwd_name(p):
    if p["form"] == "Fft":
        return "FFT+IR" if p["ir"] else "FFT"
    assert p["ir"] == 0
    direct = {"Batched": f"C{p['lpf']}", "Frame": "D"}
    if p["form"] == "Wave":
        assert p["wave"] > 0 and p["wave"] % 16 == 0
        return "WAVE" if p["rest"] == "None" else "WAVE+" + direct[p["rest"]]
    assert p["wave"] == 0 and p["rest"] == "None"
    return direct[p["form"]]


def mirror(B, T, F, hop, mode, facts, ws):
    return fz.noise_fwd_form(B, T, F, hop, mode=mode, y_aligned=facts[0] == "1", hm_aligned=facts[1] == "1", u_given=facts[2] == "1",
                             u_aligned=facts[3] == "1", workspace=ws == "0" and facts[4] == "1")


FWD_MODES = (0, 1, 2, 4, 8, 16) + tuple((l + 1) << 8 for l in range(4))
FWD_FACTS = (ALIGNED, Y_MISALIGNED, "10001", U_ALIGNED, U_MISALIGNED, "11000")


def test_forward_plan_is_what_the_python_mirror_says(dump):
    """The backward's grid (shapes x frame counts x modes x pointer facts; the frame counts straddle the group of 16 and the
    product's 4 096), with and without a workspace, and every written-out case above."""
    cases = [(1, T, F, hop, mode, facts, ws) for F, hop in BWD_SHAPES for T in (15, 16, 511, 4095, 4096, 4100) for mode in FWD_MODES
             for facts in FWD_FACTS for ws in ("0", "none")]
    cases += [c[:7] for c in FWD_CASES]
    seen = set()
    for c, p in zip(cases, dump([("f",) + c for c in cases])):
        got = fwd_name(p)
        assert got == mirror(*c), (c, p)
        if p["form"] == "Batched" or p["rest"] == "Batched":
            assert p["lpf"] == fz.noise_fwd_lpf_log(c[2], c[3], c[4]), (c, p)
        assert p["status"] == 0 or got == "D"
        seen.add(got)
    assert seen == {"FFT", "FFT+IR", "WAVE", "D"} | {f"C{l}" for l in range(4)} | {f"WAVE+C{l}" for l in range(4)}, seen


# ---- workspace size -----------------------------------------------------------------------------------------------------
def test_workspace_bytes_is_the_exported_function(dump):
    L = ddsp._lib.lib()
    shapes = [(512, 375, 257, 512), (512, 500, 65, 128), (1, 500, 195, 512), (1, 4, 195, 512), (8, 64, 195, 256), (0, 5, 195, 512),
              (2, 2100, 195, 512), (2, 300, 195, 512)]                                # test_gpu_noise_ir.py: test_workspace_contract_abi5
    got = dump([("w", B, T, F, hop, 0, ALIGNED, "none") for B, T, F, hop in shapes])
    for (B, T, F, hop), p in zip(shapes, got):
        assert p["bytes"] == L.ddsp_noise_workspace_bytes(B, T, F, hop), (B, T, F, hop)
    assert got[6]["bytes"] >= 4200 * 196 * 4 and got[7]["bytes"] > 0 and not any(p["bytes"] for p in got[:6])
