"""The inharmonic sinusoid bank without a GPU: the reference's closed form against the definition, its analytic gradients against
central differences, the tightness of its bounds at every GPU case, the planner (csrc/ddsp_sinusoids_plan.h), argument validation,
the module contract and the decoder wiring."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import ddsp_pytorch_amd as ddsp
import sinusoids_cases as cases
import sinusoids_reference as ref

SR = cases.SR
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("hop", [1, 2, 7, 8, 128])
@pytest.mark.parametrize("T", [1, 2, 5])
def test_closed_form_is_the_running_sum_of_the_interpolated_increments(T, hop):
    rng = np.random.default_rng(7 * T + hop)
    g = rng.uniform(0.0, 0.5, (2, T, 3))
    g[0, :, 0] *= np.where(np.arange(T) % 2 == 0, 1.0, 0.1)          # jumps, so that a trapezoid total at an odd hop would show
    P0 = rng.uniform(0.0, 1.0, (2, 3))
    for start in (None, P0):
        closed, summed = ref.phases_closed_form(g, hop, start), ref.phases_running_sum(g, hop, start)
        assert closed.shape == (2, T * hop, 3)
        assert (np.abs(closed - summed) <= 4 * 2.0 ** -53 * (np.abs(summed) + 1.0)).all()
    if hop % 2 == 1 and T > 1 and hop > 1:                          # the odd-hop segment total is NOT the trapezoid
        head = hop // 2
        seg = closed[:, head + hop - 1] - closed[:, head - 1] if head > 0 else None
        if seg is not None:
            trapezoid = hop * (g[:, 0] + g[:, 1]) / 2
            assert np.abs(seg - trapezoid).max() > 1e-6


def test_analytic_gradients_against_central_differences():
    B, T, K, hop = 2, 3, 2, 4
    rng = np.random.default_rng(11)
    f = rng.uniform(200.0, 7000.0, (B, T, K))
    f[0, 1, 1] = 9000.0                                              # masked, yet its g moves the phases behind it
    c = rng.uniform(0.2, 2.0, (B, T, K))
    a = rng.uniform(0.2, 1.5, (B, T, 1))
    gy = rng.standard_normal((B, T * hop))
    P0 = rng.uniform(0.0, 1.0, (B, K))
    for normalize in (True, False):
        loss = lambda f_, c_, a_: float((gy * ref.forward(f_, c_, a_, hop, SR, P0, normalize, cast=False)["y"]).sum())     # noqa: E731
        got = ref.backward(gy, f, c, a, hop, SR, P0, normalize, cast=False)
        for name, x, h in (("f", f, 1e-3), ("c", c, 1e-6), ("a", a, 1e-6)):
            num = np.zeros_like(x)
            for idx in np.ndindex(*x.shape):
                lo, hi = x.copy(), x.copy()
                lo[idx] -= h
                hi[idx] += h
                args = {"f": f, "c": c, "a": a}
                num[idx] = (loss(**{k + "_": (hi if k == name else v) for k, v in args.items()})
                            - loss(**{k + "_": (lo if k == name else v) for k, v in args.items()})) / (2 * h)
            want = got["grad_" + name]
            assert np.abs(num - want).max() <= 1e-6 * max(1.0, np.abs(want).max()), (name, normalize, np.abs(num - want).max())
        assert got["grad_c"][0, 1, 1] == 0.0 and got["grad_f"][0, 1, 1] != 0.0
    # an invalid entry: silent, and no gradient of its own
    f32 = f.astype(np.float32)
    f32[1, 0, 0] = np.nan
    got = ref.backward(gy, f32, c, a, hop, SR)
    assert got["grad_f"][1, 0, 0] == 0.0 and got["grad_c"][1, 0, 0] == 0.0 and np.isfinite(got["grad_f"]).all()


def _cap(name, value, bound, label):
    assert np.isfinite(bound).all() and (bound >= 0).all(), (label, name)
    assert bound.max() <= 1e-2 * np.abs(value).max(), (label, name, float(bound.max()), float(np.abs(value).max()))


def test_bounds_are_tight_enough_to_mean_something_at_every_gpu_case():
    """max(bound) <= 1e-2 max|value| per output tensor: a condition on the cases, not a measurement of the kernels."""
    for case in cases.forward_cases() + [cases.large_phase_case()]:
        out = ref.forward(case["f"], case["c"], case["a"], case["shape"][3], SR, normalize=case["normalize"])
        _cap("y", out["y"], out["bound"], (case["shape"], case["track"], case["normalize"]))
    for case, gy, bad in cases.backward_cases():
        out = ref.backward(gy, case["f"], case["c"], case["a"], case["shape"][3], SR, normalize=case["normalize"])
        for name in ("f", "c", "a"):
            _cap("grad_" + name, out["grad_" + name], out["bound_" + name], (case["shape"], case["track"], case["normalize"], bad is not None))


def test_silent_frames_are_silent_not_nan():
    case = cases.make_case((2, 4, 3, 8), "silent", 5)
    out = ref.forward(case["f"], case["c"], case["a"], 8, SR)
    assert np.isfinite(out["y"]).all()
    i0, i1, w0, w1 = ref.upsample_plan(4, 8)
    both_silent = np.isin(i0, (2, 3)) & np.isin(i1, (2, 3))          # frame 2 is all masked, frame 3 has c = 0
    assert both_silent.any() and (out["y"][:, both_silent] == 0.0).all() and np.abs(out["y"]).max() > 0.01


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------
def test_entry_points_validate_before_any_device_access():
    lib = ddsp._lib.lib()
    N_ = None
    word = ctypes.c_uint64(0)                                        # (a valid address; nothing is read from it)
    p = ctypes.addressof(word)
    fwd = lambda ptr, B=1, T=1, K=4, hop=4, sr=SR: lib.ddsp_sinusoids_forward(ptr, ptr, ptr, ptr, None, None, B, T, K, hop, sr, 1, None)  # noqa: E731
    bwd = lambda ptr, B=1, T=1, K=4, hop=4, sr=SR: lib.ddsp_sinusoids_backward(ptr, ptr, ptr, ptr, ptr, None, ptr, ptr, None, B, T, K, hop, sr, 1, None)  # noqa: E731
    for f in (fwd, bwd):
        assert f(N_) == -1                                           # null pointers
        assert f(N_, B=0) == 0                                       # empty batch, before the pointers
        assert f(N_, B=-1) == -1 and f(N_, B=0, T=0) == -1 and f(N_, B=0, K=0) == -1 and f(N_, hop=0) == -1 and f(N_, sr=0) == -1
        assert f(N_, hop=2048) == -1                                 # null pointers before the range
        assert f(p, hop=1025) == -2 and f(p, K=1025) == -2 and f(p, T=(1 << 22) + 1, hop=4) == -2
    assert lib.ddsp_sinusoids_supported(1024, 1024) == 1 and lib.ddsp_sinusoids_supported(1, 1) == 1
    assert lib.ddsp_sinusoids_supported(0, 8) == 0 and lib.ddsp_sinusoids_supported(1025, 8) == 0 and lib.ddsp_sinusoids_supported(8, 1025) == 0
    assert lib.ddsp_sinusoids_scratch_bytes(512, 500, 100, 128) == 0
    assert lib.ddsp_sinusoids_backward_scratch_bytes(0, 16, 16, 128, 1) == 0
    # four partials per frame and partial, four per frame, and with grad_f three more per frame and partial
    without = 4 * (4 * 16 * 4 * 10 + 4 * 16 * 4)
    assert without <= lib.ddsp_sinusoids_backward_scratch_bytes(4, 16, 10, 128, 0) <= without + 2 * 256
    assert without + 4 * 4 * 16 * 3 * 10 <= lib.ddsp_sinusoids_backward_scratch_bytes(4, 16, 10, 128, 1) <= without + 4 * 4 * 16 * 3 * 10 + 3 * 256
    assert lib.ddsp_sinusoids_set_form(1) == -2 and lib.ddsp_sinusoids_set_form(-1) == -2 and lib.ddsp_sinusoids_set_grid(2049) == -2
    assert lib.ddsp_sinusoids_set_grid(-1) == -2
    assert lib.ddsp_sinusoids_set_form(0) == 0 and lib.ddsp_sinusoids_set_grid(0) == 0


def test_hooks_refused_without_opt_in():
    code = ("import ctypes, sys; L = ctypes.CDLL(sys.argv[1]); "
            "print(L.ddsp_sinusoids_set_form(2 << 8), L.ddsp_sinusoids_set_form(0), L.ddsp_sinusoids_set_grid(2), L.ddsp_sinusoids_set_grid(0))")
    env = {k: v for k, v in os.environ.items() if k != "DDSP_TEST_HOOKS"}
    out = subprocess.run([sys.executable, "-c", code, ddsp._lib.SO_PATH], env=env, capture_output=True, text=True, check=True).stdout.split()
    assert out == ["-3", "0", "-3", "0"], out
    env["DDSP_TEST_HOOKS"] = "1"
    out = subprocess.run([sys.executable, "-c", code, ddsp._lib.SO_PATH], env=env, capture_output=True, text=True, check=True).stdout.split()
    assert out == ["0", "0", "0", "0"], out


def test_planner_through_the_dump_program(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "dump")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "ddsp-pytorch_amd", "csrc"),
                    os.path.join(ROOT, "tests", "sinusoids_plan_dump.cpp"), "-o", exe], check=True)
    # B, T, K, hop, backward, live, mode, cap
    asked = [(512, 500, 100, 128, 0, 0, 0, 0), (512, 500, 100, 128, 1, 0, 0, 0), (4, 1000, 100, 128, 0, 0, 0, 0), (4, 1000, 100, 128, 0, 1, 0, 0),
             (1, 3, 1024, 1024, 0, 0, 0, 0), (1, 3, 1024, 1024, 1, 0, 0, 0), (2, 9, 33, 64, 1, 0, (2 << 8) | (1 << 16) | (1 << 24), 2),
             (2, 4, 3, 1, 0, 0, 0, 0), (3, 700, 8, 1, 0, 0, 0, 0)]
    out = subprocess.run([exe] + [str(x) for q in asked for x in q], check=True, capture_output=True, text=True).stdout.split("\n")
    rows = [tuple(int(x) for x in line.split()) for line in out if line]
    assert len(rows) == len(asked)
    for (B, T, K, hop, bwd, live, mode, cap), (F, Tc, chunks, units, grid, tile, lds, status, scratch) in zip(asked, rows):
        assert status == 0 and 1 <= F <= min(T, 255) and Tc % F == 0 and chunks == -(-T // Tc) and units == B * chunks
        assert grid == min(units, cap or 2048) and lds <= 160 * 1024
        staged = K * (16 + 16 * F + 8 * (F + 1) + 4 * (F + 3)) + 128
        if bwd:
            assert F * K <= 256 or F == 1                            # one round of (segment, partial) items where K allows
            assert tile % 64 == 0 and 64 <= tile <= -(-(F * hop + hop // 2) // 64) * 64
            assert lds == staged + 16 * F * K + 32 * tile
        else:
            assert F == 1 or F * hop <= 512
            assert lds == staged
        if live:
            assert chunks == 1
        assert scratch >= 4 * B * T * (7 * K + 4)
    assert rows[0][:5] == (4, 128, 4, 2048, 2048)                    # 512 rows: four chunks each fill the grid
    assert rows[1][0] == 2 and rows[1][5] == 320                     # backward: two segments of 100 partials, every record in one tile
    assert rows[2][2] == 8 and rows[3][2] == 1                       # four rows are cut into 8 chunks each; a live row is one unit
    assert rows[4][0] == 1 and rows[4][6] > 64 * 1024 and rows[5][5] == 64       # the limits: one segment, the big-LDS opt-in, 64-record tiles
    assert rows[6][:3] == (1, 2, 5) and rows[6][5] == 64             # the hook's lengths
    assert rows[8][0] == 255


# ---- the module ---------------------------------------------------------------------------------------------------------------
class Conf:
    n_harmonics, n_noise_filters, sample_rate, hop_length = 8, 9, SR, 64
    decoder_mlp_units, decoder_mlp_layers, decoder_gru_units, decoder_gru_layers = 16, 2, 12, 1


def test_stretched_ratios():
    assert torch.equal(ddsp.stretched_ratios(8, 0.0), torch.arange(1, 9, dtype=torch.float32))
    r = ddsp.stretched_ratios(6, 1e-3).double()
    k = torch.arange(1, 7, dtype=torch.float64)
    assert (r - k * torch.sqrt(1 + 1e-3 * k * k)).abs().max() <= 2.0 ** -23 * 7 and bool((r[1:] / r[:-1] > k[1:] / k[:-1]).all())


def test_module_contract():
    bank = ddsp.InharmonicBank(Conf)
    assert list(bank.state_dict()) == ["inharmonicity", "detune_cents", "base_ratios"]
    assert bank.n_partials == 8 and bank.inharmonicity.requires_grad and bank.detune_cents.requires_grad
    assert bank.inharmonicity.shape == () and bank.detune_cents.shape == (8,) and float(bank.detune_cents.detach().abs().max()) == 0.0
    assert torch.equal(bank.base_ratios, torch.arange(1, 9, dtype=torch.float32))
    assert bank.phase.shape == (1, 8) and bank.phase.dtype == torch.float64
    assert torch.equal(bank.export_ratios(), torch.arange(1, 9, dtype=torch.float32))        # B = 0, no detune: the harmonic series
    fixed = ddsp.InharmonicBank(Conf, learn=False)
    assert not any(p.requires_grad for p in fixed.parameters()) and list(fixed.state_dict()) == list(bank.state_dict())
    bell = ddsp.InharmonicBank(Conf, ratios=[1.0, 2.76, 5.4, 8.93])
    assert bell.n_partials == 4 and torch.allclose(bell.export_ratios(), torch.tensor([1.0, 2.76, 5.4, 8.93]))
    stiff = ddsp.InharmonicBank(Conf, n_partials=5, inharmonicity=4e-4)
    assert torch.allclose(stiff.export_ratios(), ddsp.stretched_ratios(5, 4e-4), rtol=1e-6)
    assert torch.equal(ddsp.InharmonicBank(Conf, inharmonicity=-1.0).export_ratios(), bank.export_ratios())      # used as clamp(min=0)
    with pytest.raises(ValueError):
        ddsp.InharmonicBank(Conf, n_partials=3, ratios=[1.0, 2.0])
    # the frequencies carry the parameters' gradient, f0 none
    f0 = torch.full((1, 2, 1), 100.0, requires_grad=True)
    f = stiff.frequencies({"f0": f0})
    f.sum().backward()
    assert f.shape == (1, 2, 5) and f0.grad is None and float(stiff.inharmonicity.grad) > 0 and bool((stiff.detune_cents.grad > 0).all())
    given = torch.rand(1, 2, 5) + 1.0
    assert torch.equal(stiff.frequencies({"f0": f0, "ratios": given}), f0.detach() * given)
    x = {"f0": torch.ones(1, 2, 1), "c": torch.ones(1, 2, 8), "a": torch.ones(1, 2, 1)}
    with pytest.raises(ddsp._lib.DdspHipError):
        bank(x)                                                              # CPU tensors: no fallback
    with pytest.raises(ddsp._lib.DdspHipError):
        bank.live(x)
    with pytest.raises(ValueError):
        bank({"f0": torch.ones(1, 2), "c": torch.ones(1, 2, 8), "a": torch.ones(1, 2, 1)})
    with pytest.raises(ValueError):
        bank({"f0": torch.ones(1, 2, 1), "c": torch.ones(1, 2, 7), "a": torch.ones(1, 2, 1)})


def test_exports():
    for name in ("sinusoids", "InharmonicBank", "sinusoids_forward", "sinusoids_backward", "stretched_ratios"):
        assert name in ddsp.__all__ and hasattr(ddsp, name), name


def test_decoder_wiring():
    default = ddsp.Decoder(Conf)
    assert isinstance(default.harmonics, ddsp.OscillatorBank) and default.synth == "harmonic"
    assert "harmonics.harmonics" in default.state_dict() and not any("inharmonic" in k or "detune" in k for k in default.state_dict())
    dec = ddsp.Decoder(Conf, synth="inharmonic")
    assert isinstance(dec.harmonics, ddsp.InharmonicBank) and dec.synth == "inharmonic" and dec.harmonics.n_partials == 8
    keys = list(dec.state_dict())
    assert [k for k in keys if k.startswith("harmonics.")] == ["harmonics.inharmonicity", "harmonics.detune_cents", "harmonics.base_ratios"]
    assert [k for k in keys if not k.startswith("harmonics.")] == [k for k in default.state_dict() if not k.startswith("harmonics.")]

    class StiffConf(Conf):
        synth, inharmonicity = "inharmonic", 3e-4
    stiff = ddsp.Decoder(StiffConf)                                          # from conf.synth, with conf.inharmonicity
    assert isinstance(stiff.harmonics, ddsp.InharmonicBank) and abs(float(stiff.harmonics.inharmonicity.detach()) - 3e-4) < 1e-9
    assert isinstance(ddsp.Decoder(StiffConf, synth="harmonic").harmonics, ddsp.OscillatorBank)      # the argument wins
    with pytest.raises(ValueError, match="'harmonic', 'wavetable' or 'inharmonic'"):
        ddsp.Decoder(Conf, synth="fm")


def test_harmonic_only_entry_points_refuse_an_inharmonic_decoder():
    from encoder_common import AEConf
    ae = ddsp.AutoEncoder(AEConf, tracker="yin", synth="inharmonic")
    assert isinstance(ae.decoder.harmonics, ddsp.InharmonicBank)
    x = torch.zeros(1, 4096)
    for call in (lambda: ae.analyse(x), lambda: ae.transform(x), lambda: ae.morph(x, x)):
        with pytest.raises(ValueError, match="inharmonic"):
            call()
    with pytest.raises(ValueError, match="inharmonic"):
        ddsp.GraphedLiveDecoder(ae.decoder, 4)

    class InConf(Conf):
        synth = "inharmonic"
    with pytest.raises(ValueError, match="inharmonic"):
        ddsp.GraphedSynth(InConf, 1, 4, 9, device="cpu", live=True)
