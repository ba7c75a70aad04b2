"""Band-limited wavetables without a GPU: the fp64 reference against the truncated rfft and against its own rules, the fit rule of
csrc/ddsp_wavetable_plan.h through a small C++ program, argument validation, the module contract and the decoder wiring."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import ddsp_pytorch_amd as ddsp
import wavetable_mip_reference as mip
import wavetable_reference as ref

SR = 16000
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference against itself ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [16, 64, 512])
def test_levels_are_the_rfft_truncation(L):
    rng = np.random.default_rng(L)
    W = rng.standard_normal((3, L)).astype(np.float32)
    exact = mip.rfft_levels(W)
    n = mip.levels_of(L)
    assert n == int(np.log2(L)) + 1 and exact.shape == (n, 3, L)
    assert [mip.top_harmonic(q, L) for q in (1, n - 2, n - 1)] == [L // 4, 1, 0]
    # the fp64 direct sum with the fp64 kernels is the exact projection
    M64, _ = mip.build(W, mip.dirichlet64(L))
    assert np.abs(M64 - exact).max() <= 1e-12
    assert np.array_equal(M64[0], W.astype(np.float64))
    assert np.abs(M64[n - 1] - W.astype(np.float64).mean(1, keepdims=True)).max() <= 1e-12            # level Q: the mean alone
    # the fp32 kernels and an fp32 model of the sum (ascending i, one rounding per step) stay within the bound the build is tested
    # to; in fact within a quarter of it (0.21 at L = 16, 0.07 at L = 64, 0.02 at L = 512 with these tables)
    M, bound = mip.build(W)
    model = mip.build_fp32_model(W)
    ratio = np.abs(model[1:].astype(np.float64) - M[1:]) / bound[1:]
    print(f"L = {L}: fp32 model error / bound {ratio.max():.3f}")
    assert (bound[0] == 0).all() and np.array_equal(model[0], W) and ratio.max() <= 0.25, ratio.max()


def test_adjoint_is_the_transpose_of_the_build():
    L = 64
    rng = np.random.default_rng(5)
    W, G = rng.standard_normal((4, L)).astype(np.float32), rng.standard_normal((7, 4, L)).astype(np.float32)
    M, _ = mip.build(W)
    gW, _ = mip.adjoint(G)
    assert abs((M * G).sum() - (W * gW).sum()) <= 1e-10


def test_level_rule_is_continuous_and_strictly_safe():
    L = 512
    Q = mip.levels_of(L) - 1
    # at r = 2^e the weight of level e + 1 is exactly 1, and just below it is (almost) 1 too: continuous
    for e in range(0, Q - 1):
        r = np.float32(2.0 ** e)
        u = np.array([np.nextafter(r, np.float32(0)) / L, r / L, np.nextafter(r, np.float32(np.inf)) / L], np.float64)
        q, q1, t = mip.level_weights(u, L)
        assert q.tolist() == [e, e + 1, e + 1] and q1.tolist() == [e + 1, min(e + 2, Q), min(e + 2, Q)]
        assert t[1] == 0.0 and 1.0 - t[0] <= 2.0 ** -23 and t[2] <= 2.0 ** -22
    # u <= 0, NaN and r <= 0.5: the table as given; at and above Nyquist: the mean alone
    q, q1, t = mip.level_weights(np.array([0.0, -0.1, np.nan, 0.5 / L, 0.5, 0.7, np.inf]), L)
    assert q.tolist() == [0, 0, 0, 0, Q, Q, Q] and (t == 0).all() and q1.tolist() == [1, 1, 1, 1, Q, Q, Q]
    # level q is only heard while H_q <= 0.5 / u, over a sweep of f0 (the fp32 increments the kernels compute)
    f0 = np.geomspace(20.0, 7999.0, 4000).astype(np.float32)
    u = (f0 / np.float32(SR)).astype(np.float32).astype(np.float64)
    q, q1, t = mip.level_weights(u, L)
    H = lambda lv: np.where(lv == 0, L // 2, L >> (lv + 1))                 # noqa: E731  (level 0 holds every harmonic of the table)
    heard = np.where(t > 0, np.maximum(H(q), H(q1)), H(q))
    on = L * u > 0.5
    assert (heard[on] <= 0.5 / u[on]).all() and (q[~on] == 0).all()
    # worked figures: 440 Hz at L = 512 gives q = 4, t = 0.76; 7999 Hz plays one harmonic; 9000 Hz the mean alone
    q, q1, t = mip.level_weights(np.array([np.float32(440.0) / np.float32(SR), np.float32(7999.0) / np.float32(SR), 9000.0 / SR], np.float64), L)
    assert q[0] == 4 and abs(t[0] - 0.76) < 1e-6 and L >> (q[1] + 1) == 1 and q[2] == Q and t[2] == 0


def test_forward_reference_reduces_to_the_unlimited_one_below_half_an_entry_per_sample():
    B, T, hop, N, L = 2, 4, 8, 3, 64
    rng = np.random.default_rng(9)
    f0 = rng.uniform(20.0, 120.0, (B, T)).astype(np.float32)                 # r = 64 f0 / 16000 <= 0.48
    c, a = rng.uniform(0.1, 2.0, (B, T, N)).astype(np.float32), rng.uniform(0.1, 1.0, (B, T)).astype(np.float32)
    W = rng.standard_normal((N, L)).astype(np.float32)
    M = mip.build(W)[0].astype(np.float32)
    y, _, end = mip.forward(f0, c, a, M, hop, SR)
    y0, _, end0 = ref.forward(f0, c, a, W, hop, SR)
    assert np.array_equal(y, y0) and np.array_equal(end, end0)
    # and a sine above Nyquist is silent, below a quarter of the sample rate untouched
    h = 8
    S = np.sin(2 * np.pi * h * np.arange(L) / L)[None].astype(np.float32)
    MS = mip.build(S)[0].astype(np.float32)
    ones, amp = np.ones((1, T, 1), np.float32), np.ones((1, T), np.float32)
    loud = np.full((1, T), 1100.0, np.float32)                              # 8 x 1100 > 8000
    assert np.abs(mip.forward(loud, ones, amp, MS, hop, SR)[0]).max() <= 1e-6
    soft = np.full((1, T), 240.0, np.float32)                               # 2 x 8 x 240 <= 8000
    assert np.abs(mip.forward(soft, ones, amp, MS, hop, SR)[0] - ref.forward(soft, ones, amp, S, hop, SR)[0]).max() <= 1e-6


def test_backward_reference_equals_a_torch_restatement():
    B, T, hop, N, L = 2, 5, 16, 3, 16
    rng = np.random.default_rng(11)
    f0 = rng.uniform(300.0, 6000.0, (B, T)).astype(np.float32)
    c, a = rng.uniform(0.1, 2.0, (B, T, N)).astype(np.float32), rng.uniform(0.1, 1.0, (B, T)).astype(np.float32)
    M = mip.build(rng.standard_normal((N, L)).astype(np.float32))[0].astype(np.float32)
    gy = rng.standard_normal((B, T * hop))
    want = mip.backward(gy, f0, c, a, M, hop, SR)
    u = ref.increments(f0, hop, SR)
    q, q1, t = mip.level_weights(u, L)
    P = torch.from_numpy(ref.phases_from_increments(u))
    pos = (P - P.floor()) * L
    j = pos.floor().long().clamp(0, L - 1)
    fr = (pos - j)[..., None]
    ct, at, Mt = (torch.from_numpy(x.astype(np.float64)).requires_grad_() for x in (c, a, M))
    k = torch.arange(N)[None, None, :]
    read = lambda lv: Mt[torch.from_numpy(lv)[..., None], k, j[..., None]] * (1 - fr) + Mt[torch.from_numpy(lv)[..., None], k, ((j + 1) % L)[..., None]] * fr  # noqa: E731
    tt = torch.from_numpy(t)[..., None]
    s = (1 - tt) * read(q) + tt * read(q1)
    i0, i1, w0, w1 = ref.upsample_plan(T, hop)
    up = lambda x: torch.from_numpy(w0).reshape((1, -1) + (1,) * (x.dim() - 2)) * x[:, i0] + torch.from_numpy(w1).reshape((1, -1) + (1,) * (x.dim() - 2)) * x[:, i1]  # noqa: E731
    y = up(at) * (up(ct / ct.sum(-1, keepdim=True)) * s).sum(-1)
    assert np.abs(y.detach().numpy() - mip.forward(f0, c, a, M, hop, SR)[0]).max() <= 1e-10
    y.backward(torch.from_numpy(gy))
    assert np.abs(ct.grad.numpy() - want["grad_c"]).max() <= 1e-10
    assert np.abs(at.grad.numpy()[..., None] - want["grad_a"]).max() <= 1e-10
    assert np.abs(Mt.grad.numpy() - want["grad_M"]).max() <= 1e-10


# ---- the plan -------------------------------------------------------------------------------------------------------------------
def image_bytes(N, L):
    P4 = ((N + 3) // 4) | 1
    return 16 * (L * P4 + (L >> 4) + P4)


def test_fit_rule_through_a_host_program(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    src = tmp_path / "fit.cpp"
    src.write_text('#include <stdio.h>\n#include <stdlib.h>\n#include "ddsp_wavetable_plan.h"\n'
                   'int main(int c, char **v) { using namespace ddsp_wavetable; for (int i = 1; i + 4 < c; i += 5) {\n'
                   '  int N = atoi(v[i]), L = atoi(v[i+1]), bwd = atoi(v[i+2]), it = atoi(v[i+3]); size_t budget = (size_t)atol(v[i+4]);\n'
                   '  MipPlan p = plan_mip(4, 16, N, L, 128, bwd != 0, false, 0, 0, budget);\n'
                   '  printf("%d %d %zu %d %d %zu %d\\n", mip_levels(L), mip_fit_levels(N, L, bwd != 0, it, budget), mip_lds_bytes(N, L, 2, bwd != 0, it), '
                   'p.fit, p.walk.form, p.walk.lds_bytes, p.walk.grid); } return 0; }\n')
    exe = str(tmp_path / "fit")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "ddsp-pytorch_amd", "csrc"), str(src), "-o", exe], check=True)
    cases = [(16, 512, 0, 1024, 0), (16, 512, 1, 1024, 0), (32, 512, 0, 1024, 0), (32, 512, 1, 1024, 0), (5, 64, 0, 1024, 0),
             (5, 64, 0, 1024, 256 + 3 * image_bytes(5, 64)), (5, 64, 1, 1024, 256 + 3 * image_bytes(5, 64)), (5, 64, 0, 1024, 300),
             (4, 48, 0, 1024, 0), (64, 4096, 0, 1024, 0)]
    out = subprocess.run([exe] + [str(x) for q in cases for x in q], check=True, capture_output=True, text=True).stdout.split("\n")
    rows = [tuple(int(x) for x in line.split()) for line in out if line]
    cap = 160 * 1024
    for (N, L, bwd, it, budget), (levels, fit, two, pfit, form, lds, grid) in zip(cases, rows):
        have = budget if budget else cap
        want_levels = int(np.log2(L)) + 1 if L & (L - 1) == 0 and 16 <= L <= 4096 else 0
        assert levels == want_levels
        need = lambda n: 256 + n * image_bytes(N, L) + (32 * it if bwd else 0)         # noqa: E731
        want_fit = max([n for n in range(0, levels + 1) if need(n) <= have] or [0])
        assert fit == want_fit and two == need(2)
        assert pfit == (want_fit if want_fit >= 2 else 0) and form == (1 if pfit else 2) and lds == need(pfit) and lds <= cap
    by = {c[:3] + (c[4],): r for c, r in zip(cases, rows)}
    assert by[(16, 512, 0, 0)][3] == 3 and by[(16, 512, 1, 0)][3] == 3        # the flagship shape: three levels beside the records
    assert by[(32, 512, 0, 0)][3] == 2 and by[(32, 512, 1, 0)][3] == 0        # 32 tables: two levels in the forward, none in the backward
    assert by[(5, 64, 0, 0)][3] == 7                                          # small tables: the whole pyramid
    assert by[(4, 48, 0, 0)][0] == 0 and by[(64, 4096, 0, 0)][3] == 0


def test_form_query_and_hooks():
    lib = ddsp._lib.lib()
    form = lambda N, L, hop=128, B=4, T=16: lib.ddsp_wavetable_form_bl(B, T, N, L, hop)            # noqa: E731
    assert lib.ddsp_wavetable_set_form(0) == 0 and lib.ddsp_wavetable_set_mip_lds(0) == 0
    LDS, GLOBAL = 1, 2
    assert form(16, 512) == LDS | (LDS << 2) | (3 << 8) | (3 << 16)
    assert form(32, 512) == LDS | (GLOBAL << 2) | (2 << 8)
    assert form(5, 64) == LDS | (LDS << 2) | (7 << 8) | (7 << 16)
    assert form(4, 48) == -2 and form(1, 8192) == -2 and form(4, 8) == -2 and form(0, 64) == -1 and form(4, 64, hop=2048) == -2
    assert lib.ddsp_wavetable_mip_levels(512) == 10 and lib.ddsp_wavetable_mip_levels(16) == 5 and lib.ddsp_wavetable_mip_levels(4096) == 13
    assert lib.ddsp_wavetable_mip_levels(48) == -2 and lib.ddsp_wavetable_mip_levels(8) == -2 and lib.ddsp_wavetable_mip_levels(8192) == -2
    try:
        assert lib.ddsp_wavetable_set_form(2) == 0 and form(16, 512) == GLOBAL | (GLOBAL << 2)
        assert lib.ddsp_wavetable_set_form(1) == 0 and form(5, 64) & 15 == LDS | (LDS << 2) and form(16, 512) == -2   # all levels or refused
        assert lib.ddsp_wavetable_set_form(0) == 0
        assert lib.ddsp_wavetable_set_mip_lds(256 + 3 * image_bytes(5, 64) + 32 * 128) == 0
        assert form(5, 64, hop=8) == LDS | (LDS << 2) | (4 << 8) | (3 << 16)      # (the backward's 128 records take a level's room)
        assert lib.ddsp_wavetable_set_mip_lds(300) == 0 and form(5, 64) == GLOBAL | (GLOBAL << 2)
        assert lib.ddsp_wavetable_set_mip_lds(-1) == -2 and lib.ddsp_wavetable_set_mip_lds(160 * 1024 + 1) == -2
        # the unlimited plan never sees the new hook
        assert lib.ddsp_wavetable_form(4, 16, 16, 512, 128) == LDS | (LDS << 2)
    finally:
        assert lib.ddsp_wavetable_set_form(0) == 0 and lib.ddsp_wavetable_set_mip_lds(0) == 0
    # the scratch: the partials of every frame, one private [Q+1, N, L] table per workgroup (8 here) and their masks
    need = 4 * (4 * 16 * 3 * 16 + 4 * 16 * 3 + 8 * 10 * 16 * 512 + 8)
    assert need <= lib.ddsp_wavetable_backward_bl_scratch_bytes(4, 16, 16, 512, 128) <= need + 4 * 256
    # ... and never more than 512 MiB of private tables: 2^18 entries in 13 levels leave 39 workgroups of the 256
    big = lib.ddsp_wavetable_backward_bl_scratch_bytes(512, 16, 64, 4096, 128)
    assert 39 * 13 * 4 * 2 ** 18 <= big <= 512 * 2 ** 20 + 4 * (512 * 16 * 3 * 65) + 4 * 256
    assert lib.ddsp_wavetable_backward_bl_scratch_bytes(4, 16, 4, 48, 128) == 0 and lib.ddsp_wavetable_scratch_bytes(4, 16, 16, 512, 128) == 0


def test_hook_refused_without_opt_in():
    code = ("import ctypes, sys; L = ctypes.CDLL(sys.argv[1]); L.ddsp_wavetable_set_mip_lds.argtypes = [ctypes.c_long]; "
            "print(L.ddsp_wavetable_set_mip_lds(4096), L.ddsp_wavetable_set_mip_lds(0), L.ddsp_wavetable_form_bl(4, 16, 16, 512, 128))")
    env = {k: v for k, v in os.environ.items() if k != "DDSP_TEST_HOOKS"}
    out = subprocess.run([sys.executable, "-c", code, ddsp._lib.SO_PATH], env=env, capture_output=True, text=True, check=True).stdout.split()
    assert out == ["-3", "0", str(1 | (1 << 2) | (3 << 8) | (3 << 16))], out


def test_entry_points_validate_before_any_device_access():
    lib = ddsp._lib.lib()
    N_ = None
    word = ctypes.c_uint64(0)                                    # (a valid address; nothing is read from it)
    p = ctypes.addressof(word)
    fwd = lambda ptr, B=1, T=1, N=4, L=16, hop=4, sr=SR: lib.ddsp_wavetable_forward_bl(ptr, ptr, ptr, ptr, ptr, None, B, T, N, L, hop, sr, None)  # noqa: E731
    bwd = lambda ptr, B=1, T=1, N=4, L=16, hop=4, sr=SR: lib.ddsp_wavetable_backward_bl(ptr, ptr, ptr, ptr, ptr, None, ptr, ptr, ptr, ptr, B, T, N, L, hop, sr, None)  # noqa: E731
    for f in (fwd, bwd):
        assert f(N_) == -1 and f(N_, B=0) == 0 and f(N_, B=-1) == -1 and f(N_, B=0, T=0) == -1 and f(N_, sr=0) == -1
        assert f(N_, L=48) == -1                                 # null pointers before the range
        assert f(p, L=48) == -2 and f(p, L=8192) == -2 and f(p, L=8) == -2 and f(p, hop=2048) == -2 and f(p, N=1025) == -2
    for f in (lib.ddsp_wavetable_mip_build, lib.ddsp_wavetable_mip_adjoint):
        assert f(N_, N_, N_, 4, 64, None) == -1 and f(p, p, p, 0, 64, None) == -1
        assert f(p, p, p, 4, 48, None) == -2 and f(p, p, p, 1, 8192, None) == -2 and f(p, p, p, 4, 8, None) == -2
        assert f(p, p, p, 128, 4096, None) == -2                 # N L > 2^18
    # the symbols sit behind the unlimited wavetable's, in the header's order, and the ABI number is unchanged
    names = list(ddsp._lib.SIGNATURES)
    at = names.index("ddsp_wavetable_set_grid")
    assert names[at + 1:at + 9] == ["ddsp_wavetable_mip_levels", "ddsp_wavetable_mip_build", "ddsp_wavetable_mip_adjoint", "ddsp_wavetable_form_bl",
                                    "ddsp_wavetable_forward_bl", "ddsp_wavetable_backward_bl_scratch_bytes", "ddsp_wavetable_backward_bl",
                                    "ddsp_wavetable_set_mip_lds"]
    assert ddsp._lib.ABI_VERSION == 5 == lib.ddsp_hip_abi_version()


# ---- the module -------------------------------------------------------------------------------------------------------------------
class Conf:
    n_harmonics, n_noise_filters, sample_rate, hop_length = 8, 9, SR, 64
    decoder_mlp_units, decoder_mlp_layers, decoder_gru_units, decoder_gru_layers = 16, 2, 12, 1


def test_dirichlet_kernels_are_the_reference_and_cached():
    for L in (16, 64, 512):
        D = ddsp.dirichlet_kernels(L)
        assert D.dtype == torch.float32 and tuple(D.shape) == (mip.levels_of(L), L)
        assert np.abs(D.numpy().astype(np.float64) - mip.dirichlet64(L)).max() <= 2.0 ** -24 * 1.001      # fl32 of the fp64 value (|D| <= 1)
        assert ddsp.dirichlet_kernels(L) is D
    for bad in (48, 8, 8192):
        with pytest.raises(ValueError, match="power of two"):
            ddsp.dirichlet_kernels(bad)


def test_module_contract():
    off = ddsp.WavetableBank(Conf, table_size=64)
    on = ddsp.WavetableBank(Conf, table_size=64, band_limited=True)
    assert off.band_limited is False and on.band_limited is True
    assert list(on.state_dict()) == list(off.state_dict()) == ["wavetables"]                 # the pyramid and the kernels are not persistent
    assert [n for n, _ in on.named_buffers()] == [n for n, _ in off.named_buffers()] and len(list(on.parameters())) == 1
    assert torch.equal(on.wavetables, off.wavetables)
    off.load_state_dict(on.state_dict())
    given = torch.randn(8, 64)
    on.load_tables(given)
    assert torch.equal(on.export_tables(), given)

    class BlConf(Conf):
        wavetable_band_limited, wavetable_size = True, 64
    assert ddsp.WavetableBank(BlConf).band_limited is True
    assert ddsp.WavetableBank(BlConf, band_limited=False).band_limited is False             # the argument wins
    assert ddsp.WavetableBank(Conf).band_limited is False                                    # default: off
    for bad in (48, 8192):
        with pytest.raises(ValueError, match="power of two"):
            ddsp.WavetableBank(Conf, table_size=bad, init=torch.zeros(8, bad), band_limited=True)
        with pytest.raises(ValueError, match="power of two"):
            ddsp.wavetable_mipmaps(torch.zeros(2, bad))
    assert ddsp.WavetableBank(Conf, table_size=48, init=torch.zeros(8, 48)).table_size == 48     # the unlimited path keeps its own range
    x = {"f0": torch.ones(1, 2, 1), "c": torch.ones(1, 2, 8), "a": torch.ones(1, 2, 1)}
    with pytest.raises(ddsp._lib.DdspHipError):
        on(x)                                                                                # CPU tensors: no fallback
    with pytest.raises(ddsp._lib.DdspHipError):
        on.live(x)
    with pytest.raises(ddsp._lib.DdspHipError):
        ddsp.wavetable_mipmaps(torch.zeros(2, 64))


def test_decoder_wiring():
    class WtConf(Conf):
        synth, n_wavetables, wavetable_size = "wavetable", 5, 32
    plain = ddsp.Decoder(WtConf)
    assert plain.harmonics.band_limited is False
    dec = ddsp.Decoder(WtConf, band_limited=True)
    assert isinstance(dec.harmonics, ddsp.WavetableBank) and dec.harmonics.band_limited is True
    assert list(dec.state_dict()) == list(plain.state_dict())

    class BlConf(WtConf):
        wavetable_band_limited = True
    assert ddsp.Decoder(BlConf).harmonics.band_limited is True and ddsp.Decoder(BlConf, band_limited=False).harmonics.band_limited is False
    assert isinstance(ddsp.Decoder(BlConf, synth="harmonic").harmonics, ddsp.OscillatorBank)
    with pytest.raises(ValueError, match="power of two"):
        class Odd(BlConf):
            wavetable_size = 48
        ddsp.Decoder(Odd)
    from encoder_common import AEConf

    class WtAE(AEConf):
        wavetable_size = 64
    ae = ddsp.AutoEncoder(WtAE, tracker="yin", synth="wavetable", band_limited=True)
    assert ae.decoder.harmonics.band_limited is True
    with pytest.raises(ValueError, match="wavetable"):                                       # the refusals stay
        ae.analyse(torch.zeros(1, 4096))
    with pytest.raises(ValueError, match="wavetable"):
        ddsp.GraphedLiveDecoder(ae.decoder, 4)
