"""Wavetable synthesis without a GPU: the fp64 reference against a torch restatement with autograd, the definition's limits, the
planner (csrc/ddsp_wavetable_plan.h through ddsp_wavetable_form), argument validation, the module contract and the decoder wiring."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ddsp_pytorch_amd as ddsp
import wavetable_reference as ref

SR = 16000


def random_case(B, T, hop, N, L, seed, f_lo=100.0, f_hi=3000.0):
    rng = np.random.default_rng(seed)
    return dict(f0=rng.uniform(f_lo, f_hi, (B, T)).astype(np.float32), c=rng.uniform(0.05, 2.0, (B, T, N)).astype(np.float32),
                a=rng.uniform(0.1, 1.5, (B, T)).astype(np.float32), W=rng.standard_normal((N, L)).astype(np.float32), hop=hop)


def torch_forward(u, c, a, W, hop, P0=None):
    """The definition as torch operations in fp64, from the increments u [B, n] on: autograd gives the three gradients."""
    up = lambda x: F.interpolate(x.transpose(1, 2), scale_factor=hop, mode="linear", align_corners=False).transpose(1, 2)   # noqa: E731
    L = W.shape[1]
    P = torch.cumsum(u, 1) + (0.0 if P0 is None else P0[:, None])
    pos = (P - P.floor()) * L
    j = pos.floor().long().clamp(0, L - 1)
    fr = pos - j
    s = W[:, j].permute(1, 2, 0) + fr[..., None] * (W[:, (j + 1) % L] - W[:, j]).permute(1, 2, 0)
    wn = c / c.sum(-1, keepdim=True)
    return up(a[..., None])[..., 0] * (up(wn) * s).sum(-1)


def test_reference_equals_a_torch_fp64_restatement():
    case = random_case(2, 5, 16, 4, 16, seed=1)      # (a power-of-two hop: the fp32 upsampling weights are exact, so fp64 F.interpolate has them too)
    hop = case["hop"]
    gy = np.random.default_rng(2).standard_normal((2, 5 * hop))
    y, _, _ = ref.forward(case["f0"], case["c"], case["a"], case["W"], hop, SR)
    g = ref.backward(gy, case["f0"], case["c"], case["a"], case["W"], hop, SR)
    u = torch.from_numpy(ref.increments(case["f0"], hop, SR))
    c, a, W = (torch.from_numpy(case[k].astype(np.float64)).requires_grad_() for k in ("c", "a", "W"))
    yt = torch_forward(u, c, a, W, hop)
    yt.backward(torch.from_numpy(gy))
    assert np.abs(yt.detach().numpy() - y).max() <= 1e-10
    assert np.abs(c.grad.numpy() - g["grad_c"]).max() <= 1e-10
    assert np.abs(a.grad.numpy()[..., None] - g["grad_a"]).max() <= 1e-10
    assert np.abs(W.grad.numpy() - g["grad_W"]).max() <= 1e-10
    # the fp32 upsampling of the reference is F.interpolate's own
    i0, i1, w0, w1 = ref.upsample_plan(5, hop)
    x = torch.randn(1, 1, 5, generator=torch.Generator().manual_seed(4))
    want = F.interpolate(x, scale_factor=hop, mode="linear", align_corners=False)[0, 0].numpy().astype(np.float64)
    got = w0 * x[0, 0].numpy().astype(np.float64)[i0] + w1 * x[0, 0].numpy().astype(np.float64)[i1]
    assert np.abs(got - want).max() <= 2.0 ** -23 * float(x.abs().max())        # (the fp32 result's own rounding)


def test_one_sine_table_is_a_sine_within_the_interpolation_error():
    L, hop, T = 4096, 64, 6
    W = np.sin(2 * np.pi * np.arange(L) / L)[None].astype(np.float64)
    f0 = np.linspace(200.0, 900.0, T, dtype=np.float32)[None]
    a = np.full((1, T), 0.8, np.float32)
    y, _, _ = ref.forward(f0, np.ones((1, T, 1), np.float32), a, W, hop, SR)
    P = ref.phases(f0, hop, SR)
    assert np.abs(y - 0.8 * np.sin(2 * np.pi * P)).max() <= 0.8 * (2 * np.pi / L) ** 2 / 8 + 1e-12


def test_carried_phase_two_halves_equal_one_pass():
    """The reference's P0 path -- the oracle of the GPU live test: a second block started from the first block's end phase walks the
    same phases (modulo whole cycles) as one pass over the same increments, and its output is the torch restatement's from P0."""
    case = random_case(3, 8, 10, 3, 32, seed=3)
    hop, half = case["hop"], 4
    u = ref.increments(case["f0"], hop, SR)
    n = half * hop
    one_pass = ref.phases_from_increments(u)
    first = ref.phases_from_increments(u[:, :n])
    assert np.array_equal(first, one_pass[:, :n])
    end1 = first[:, -1] - np.floor(first[:, -1])
    second = ref.phases_from_increments(u[:, n:], P0=end1)
    assert (second[:, 0] < 2.0).all() and (one_pass[:, n] > 2.0).any()                  # (restarted inside [0, 1), not at P[n])
    d = np.abs((second - np.floor(second)) - (one_pass[:, n:] - np.floor(one_pass[:, n:])))
    assert np.minimum(d, 1 - d).max() <= 1e-12
    # forward() hands exactly that phase on, and starts from it: block 2 from P0 against the torch restatement started from P0
    f1, f2 = case["f0"][:, :half], case["f0"][:, half:]
    _, _, e1 = ref.forward(f1, case["c"][:, :half], case["a"][:, :half], case["W"], hop, SR)
    p1 = ref.phases(f1, hop, SR)[:, -1]
    assert np.array_equal(e1, p1 - np.floor(p1))
    assert np.array_equal(ref.phases(f2, hop, SR, P0=e1), ref.phases_from_increments(ref.increments(f2, hop, SR), P0=e1))
    y2, _, e2 = ref.forward(f2, case["c"][:, half:], case["a"][:, half:], case["W"], hop, SR, P0=e1)
    tens = lambda x: torch.from_numpy(np.asarray(x, np.float64))          # noqa: E731
    # (hop 10: the restatement takes the reference's fp32 upsampling weights, which fp64 F.interpolate does not have)
    i0, i1, w0, w1 = ref.upsample_plan(half, hop)
    P = torch.cumsum(tens(ref.increments(f2, hop, SR)), 1) + tens(e1)[:, None]
    pos = (P - P.floor()) * 32
    j = pos.floor().long().clamp(0, 31)
    W = tens(case["W"])
    s = (W[:, j] + (pos - j) * (W[:, (j + 1) % 32] - W[:, j])).permute(1, 2, 0)
    c2 = tens(case["c"][:, half:])
    wn = c2 / c2.sum(-1, keepdim=True)
    up = lambda x: tens(w0).reshape((1, -1) + (1,) * (x.dim() - 2)) * x[:, i0] + tens(w1).reshape((1, -1) + (1,) * (x.dim() - 2)) * x[:, i1]   # noqa: E731
    want = up(tens(case["a"][:, half:])) * (up(wn) * s).sum(-1)
    assert np.abs(y2 - want.numpy()).max() <= 1e-10
    last = P[:, -1].numpy()
    assert np.abs(e2 - (last - np.floor(last))).max() <= 1e-12 and ((0.0 <= e2) & (e2 < 1.0)).all()
    # a start phase matters: the same block from zero sounds different
    y0, _, _ = ref.forward(f2, case["c"][:, half:], case["a"][:, half:], case["W"], hop, SR)
    assert np.abs(y0 - y2).max() > 1e-3


# ---- the planner ------------------------------------------------------------------------------------------------------------
def image_bytes(N, L):
    P4 = ((N + 3) // 4) | 1
    return 16 * (L * P4 + (L >> 4) + P4)


def test_planner_forms_at_the_lds_limit():
    lib = ddsp._lib.lib()
    form = lambda N, L, hop=128, B=4, T=16: lib.ddsp_wavetable_form(B, T, N, L, hop)       # noqa: E731
    LDS, GLOBAL = 1, 2
    assert lib.ddsp_wavetable_set_form(0) == 0
    assert form(16, 512) == LDS | (LDS << 2)
    assert form(100, 512) == GLOBAL | (GLOBAL << 2)              # 205 KB of tables: from memory
    # the backward holds two images and the iteration's records: 32 tables of 512 points fit it with shorter iterations (3 frames
    # of hop 128), 40 tables fit the forward alone
    assert form(32, 512) == LDS | (LDS << 2)
    assert form(40, 512) == LDS | (GLOBAL << 2)
    # at the limit: head (256 bytes) + image <= 160 KiB
    budget = 160 * 1024 - 256
    N = 36                                                       # pitch 9 units of 16 bytes
    L_fit = max(L for L in range(2, 4096) if image_bytes(N, L) <= budget)
    assert image_bytes(N, L_fit) <= budget < image_bytes(N, L_fit + 1)
    assert form(N, L_fit) & 3 == LDS and form(N, L_fit + 1) & 3 == GLOBAL
    # bad shapes and shapes out of range
    assert form(0, 512) == -1 and form(4, 1) == -1 and form(4, 8, hop=0) == -1 and form(4, 8, T=0) == -1 and form(4, 8, B=0) == -1
    assert form(1025, 8) == -2 and form(4, 65537) == -2 and form(1024, 512) == -2 and form(4, 8, hop=1025) == -2
    assert form(4, 8, hop=1024, T=(1 << 14) + 1) == -2           # T hop > 2^24
    assert lib.ddsp_wavetable_supported(32, 512) == 1 and lib.ddsp_wavetable_supported(0, 512) == 0
    assert lib.ddsp_wavetable_supported(1024, 512) == 0 and lib.ddsp_wavetable_supported(8, 1) == 0
    # the hook forces either form; the LDS form where it does not fit is out of range
    assert lib.ddsp_wavetable_set_form(2) == 0 and form(16, 512) == GLOBAL | (GLOBAL << 2)
    assert lib.ddsp_wavetable_set_form(1) == 0 and form(16, 512) == LDS | (LDS << 2) and form(100, 512) == -2
    assert lib.ddsp_wavetable_set_form(3) == -2 and lib.ddsp_wavetable_set_form(4) == -2 and lib.ddsp_wavetable_set_form(-1) == -2
    assert lib.ddsp_wavetable_set_grid(257) == -2 and lib.ddsp_wavetable_set_grid(-1) == -2
    assert lib.ddsp_wavetable_set_form(0) == 0 and lib.ddsp_wavetable_set_grid(0) == 0


def test_plan_header_compiles_on_its_own(tmp_path):
    """The planner is plain C++: a host program reads the same plans the library answers with."""
    import shutil
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    src = tmp_path / "dump.cpp"
    src.write_text('#include <stdio.h>\n#include <stdlib.h>\n#include "ddsp_wavetable_plan.h"\n'
                   'int main(int c, char **v) { using namespace ddsp_wavetable; for (int i = 1; i + 5 < c; i += 6) {\n'
                   '  Plan p = plan(atol(v[i]), atol(v[i+1]), atoi(v[i+2]), atoi(v[i+3]), atoi(v[i+4]), atoi(v[i+5]) != 0, false, 0, 0);\n'
                   '  printf("%d %d %d %d %ld %d %d %zu %d\\n", p.form, p.iter_frames, p.chunk_frames, p.chunks, p.units, p.grid, p.parts, '
                   'p.lds_bytes, p.status); } return 0; }\n')
    exe = str(tmp_path / "dump")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", os.path.join(root, "ddsp-pytorch_amd", "csrc"), str(src), "-o", exe], check=True)
    cases = [(512, 500, 16, 512, 128, 0), (512, 500, 32, 512, 128, 1), (4, 1000, 16, 512, 128, 0), (1, 3, 100, 64, 5, 1)]
    out = subprocess.run([exe] + [str(x) for q in cases for x in q], check=True, capture_output=True, text=True).stdout.split("\n")
    rows = [tuple(int(x) for x in line.split()) for line in out if line]
    lib = ddsp._lib.lib()
    for (B, T, N, L, hop, bwd), (form, F_, Tc, chunks, units, grid, parts, lds, status) in zip(cases, rows):
        assert status == 0 and form == (lib.ddsp_wavetable_form(B, T, N, L, hop) >> (2 * bwd)) & 3
        assert F_ * hop <= 1024 and Tc % F_ == 0 and chunks == -(-T // Tc) and units == B * chunks and grid == min(units, 256)
        assert lds <= 160 * 1024 and parts in (1, 2, 4, 8, 16, 32, 64) and F_ * (((N + 3) // 4 | 1) + 1) * parts <= 1024
    assert rows[0][3] == 1 and rows[2][3] == 8                   # 512 rows fill the grid; 4 rows are cut into 8 chunks each


def test_entry_points_validate_before_any_device_access():
    lib = ddsp._lib.lib()
    N_ = None
    word = ctypes.c_uint64(0)                                    # (a valid address; nothing is read from it)
    p = ctypes.addressof(word)
    fwd = lambda ptr, B=1, T=1, N=4, L=8, hop=4, sr=SR: lib.ddsp_wavetable_forward(ptr, ptr, ptr, ptr, ptr, None, None, B, T, N, L, hop, sr, None)  # noqa: E731
    bwd = lambda ptr, B=1, T=1, N=4, L=8, hop=4, sr=SR: lib.ddsp_wavetable_backward(ptr, ptr, ptr, ptr, ptr, None, ptr, ptr, ptr, ptr, B, T, N, L, hop, sr, None)  # noqa: E731
    for f in (fwd, bwd):
        assert f(N_) == -1                                       # null pointers
        assert f(N_, B=0) == 0                                   # empty batch, before the pointers
        assert f(N_, B=-1) == -1 and f(N_, B=0, T=0) == -1 and f(N_, B=0, L=1) == -1 and f(N_, sr=0) == -1   # a bad shape first of all
        assert f(N_, hop=2048) == -1                             # null pointers before the range
        assert f(p, hop=2048) == -2 and f(p, N=1025) == -2 and f(p, N=1024, L=512) == -2 and f(p, T=1 << 23, hop=4) == -2
    assert lib.ddsp_wavetable_scratch_bytes(4, 16, 16, 512, 128) == 0
    assert lib.ddsp_wavetable_backward_scratch_bytes(0, 16, 16, 512, 128) == 0
    # the partials of every frame and one private table per workgroup of the plan: 4 rows x 2 chunks here, not the cap of 256
    need = 4 * (4 * 16 * 3 * 16 + 4 * 16 * 3 + 8 * 16 * 512)
    assert need <= lib.ddsp_wavetable_backward_scratch_bytes(4, 16, 16, 512, 128) <= need + 3 * 256
    assert lib.ddsp_wavetable_backward_scratch_bytes(512, 16, 16, 512, 128) >= 4 * 256 * 16 * 512


def test_hooks_refused_without_opt_in():
    code = ("import ctypes, sys; L = ctypes.CDLL(sys.argv[1]); "
            "print(L.ddsp_wavetable_set_form(1), L.ddsp_wavetable_set_form(0), L.ddsp_wavetable_set_grid(2), L.ddsp_wavetable_set_grid(0), "
            "L.ddsp_wavetable_form(4, 16, 16, 512, 128))")
    env = {k: v for k, v in os.environ.items() if k != "DDSP_TEST_HOOKS"}
    out = subprocess.run([sys.executable, "-c", code, ddsp._lib.SO_PATH], env=env, capture_output=True, text=True, check=True).stdout.split()
    assert out == ["-3", "0", "-3", "0", "5"], out
    env["DDSP_TEST_HOOKS"] = "1"
    out = subprocess.run([sys.executable, "-c", code, ddsp._lib.SO_PATH], env=env, capture_output=True, text=True, check=True).stdout.split()
    assert out == ["0", "0", "0", "0", "5"], out


# ---- the module ---------------------------------------------------------------------------------------------------------------
class Conf:
    n_harmonics, n_noise_filters, sample_rate, hop_length = 8, 9, SR, 64
    decoder_mlp_units, decoder_mlp_layers, decoder_gru_units, decoder_gru_layers = 16, 2, 12, 1


def test_module_contract():
    wt = ddsp.WavetableBank(Conf, table_size=64)
    assert list(wt.state_dict()) == ["wavetables"] and wt.wavetables.requires_grad and wt.wavetables.shape == (8, 64)
    k, j = np.arange(1, 9)[:, None], np.arange(64)[None, :]
    assert np.abs(wt.wavetables.detach().numpy() - np.sin(2 * np.pi * k * j / 64)).max() <= 1e-7
    assert ddsp.WavetableBank(Conf).wavetables.shape == (8, 512)             # defaults: conf.n_harmonics tables of 512 points

    class Sized(Conf):
        n_wavetables, wavetable_size = 5, 32
    assert ddsp.WavetableBank(Sized).wavetables.shape == (5, 32)
    assert ddsp.WavetableBank(Sized, n_wavetables=3, table_size=16).wavetables.shape == (3, 16)
    with pytest.raises(ValueError):
        ddsp.WavetableBank(Conf, table_size=16)                              # 2 N >= L: harmonic 8 does not fit 16 points
    with pytest.raises(ValueError):
        ddsp.WavetableBank(Conf, init="noise")
    with pytest.raises(ValueError):
        ddsp.WavetableBank(Conf, table_size=16, init=torch.zeros(8, 17))
    given = torch.randn(8, 16)
    assert torch.equal(ddsp.WavetableBank(Conf, table_size=16, init=given).wavetables.detach(), given)
    x = {"f0": torch.ones(1, 2, 1), "c": torch.ones(1, 2, 8), "a": torch.ones(1, 2, 1)}
    with pytest.raises(ddsp._lib.DdspHipError):
        wt(x)                                                                # CPU tensors: no fallback
    with pytest.raises(ddsp._lib.DdspHipError):
        wt.live(x)
    with pytest.raises(ValueError):
        wt({"f0": torch.ones(1, 2), "c": torch.ones(1, 2, 8), "a": torch.ones(1, 2, 1)})


def test_export_and_load_tables():
    wt = ddsp.WavetableBank(Conf, table_size=64, init=torch.randn(8, 64))
    t = wt.export_tables()
    assert t.device.type == "cpu" and t.shape == (8, 64) and torch.equal(t, wt.wavetables.detach())
    other = ddsp.WavetableBank(Conf, table_size=64)
    other.load_tables(t)
    assert torch.equal(other.wavetables.detach(), t)                         # equal L: to the bit
    assert other.wavetables.requires_grad
    # another L: read linearly on the circle.  A sine survives within the interpolation error, the last point reads towards entry 0
    fine = ddsp.WavetableBank(Conf, table_size=256)
    coarse = ddsp.WavetableBank(Conf, table_size=64)
    coarse.load_tables(fine.export_tables())
    k, j = np.arange(1, 9)[:, None], np.arange(64)[None, :]
    assert np.abs(coarse.wavetables.detach().numpy() - np.sin(2 * np.pi * k * j / 64)).max() <= 1e-6          # 256 / 64 is whole
    up = ddsp.WavetableBank(Conf, table_size=96)
    up.load_tables(fine.export_tables()[:, ::4].contiguous())                # 64 -> 96 points
    k, j = np.arange(1, 9)[:, None], np.arange(96)[None, :]
    assert np.abs(up.wavetables.detach().numpy() - np.sin(2 * np.pi * k * j / 96)).max() <= (2 * np.pi * 8 / 64) ** 2 / 8 + 1e-6
    with pytest.raises(ValueError):
        up.load_tables(torch.zeros(7, 64))


DECODER_KEYS = (
    [f"controller.{s}.mlp_layer{i}.{m}" for s in ("mlp_f0", "mlp_loudness") for i in (1, 2) for m in ("0.weight", "0.bias", "1.weight", "1.bias")]
    + [f"controller.gru.{n}_l0" for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    + [f"controller.mlp_gru.mlp_layer{i}.{m}" for i in (1, 2) for m in ("0.weight", "0.bias", "1.weight", "1.bias")]
    + [f"controller.{h}.{m}" for h in ("dense_harmonic", "dense_loudness", "dense_filter") for m in ("weight", "bias")]
    + ["harmonics.harmonics", "harmonics.last_phases", "reverb.noise", "reverb.decay", "reverb.wet", "reverb.t", "reverb.buffer"])


def test_default_decoder_is_unchanged():
    dec = ddsp.Decoder(Conf)
    assert list(dec.state_dict()) == DECODER_KEYS
    assert isinstance(dec.harmonics, ddsp.OscillatorBank) and dec.synth == "harmonic"
    assert list(ddsp.Decoder(Conf, synth="harmonic").state_dict()) == DECODER_KEYS


def test_wavetable_decoder_wiring():
    class WtConf(Conf):
        synth, n_wavetables, wavetable_size = "wavetable", 5, 32
    dec = ddsp.Decoder(WtConf)                                               # from conf.synth
    assert isinstance(dec.harmonics, ddsp.WavetableBank) and dec.harmonics.wavetables.shape == (5, 32)
    assert dec.controller.dense_harmonic.out_features == 5                   # the controller mixes the tables
    keys = list(dec.state_dict())
    assert "harmonics.wavetables" in keys and "harmonics.harmonics" not in keys and "harmonics.last_phases" not in keys
    assert isinstance(ddsp.Decoder(Conf, synth="wavetable").harmonics, ddsp.WavetableBank)
    assert isinstance(ddsp.Decoder(WtConf, synth="harmonic").harmonics, ddsp.OscillatorBank)     # the argument wins
    with pytest.raises(ValueError):
        ddsp.Decoder(Conf, synth="fm")


def test_harmonic_only_entry_points_refuse_a_wavetable_decoder():
    from encoder_common import AEConf

    class WtAE(AEConf):
        wavetable_size = 64
    ae = ddsp.AutoEncoder(WtAE, tracker="yin", synth="wavetable")
    assert isinstance(ae.decoder.harmonics, ddsp.WavetableBank)
    x = torch.zeros(1, 4096)
    for call in (lambda: ae.analyse(x), lambda: ae.transform(x), lambda: ae.morph(x, x)):
        with pytest.raises(ValueError, match="wavetable"):
            call()
    with pytest.raises(ValueError, match="wavetable"):
        ddsp.GraphedLiveDecoder(ae.decoder, 4)

    class WtConf(Conf):
        synth = "wavetable"
    with pytest.raises(ValueError, match="wavetable"):
        ddsp.GraphedSynth(WtConf, 1, 4, 9, device="cpu", live=True)
