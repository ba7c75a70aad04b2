"""CPU-side checks: the C-ABI library loads and exports every symbol include/ddsp_hip.h declares
(no compute calls without a GPU), argument validation, host logic, state-dict compatibility."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ddsp_pytorch_amd as ddsp
from ddsp_pytorch_amd import synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Conf:
    def __init__(self, n_harmonics, sample_rate, hop_length):
        self.n_harmonics, self.sample_rate, self.hop_length = n_harmonics, sample_rate, hop_length


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "ddsp_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(ddsp_[a-z0-9_]+)\s*\(", text)))


C_TYPES = {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "long": ctypes.c_long, "size_t": ctypes.c_size_t,
           "uint64_t": ctypes.c_uint64, "float": ctypes.c_float, "double": ctypes.c_double}


def declared_prototypes():
    """-> {name: (return type, [(base type, is pointer)])} of every declaration in include/ddsp_hip.h ("const" and names dropped)."""
    text = open(os.path.join(ROOT, "include", "ddsp_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = {}
    for ret, name, params in re.findall(r"(\w+)\s+(ddsp_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        args = []
        for param in params.split(","):
            words = param.replace("*", " * ").split()
            if words == ["void"]:
                continue
            words = [w for w in words if w != "const"]
            assert len([w for w in words if w != "*"]) == 2, (name, param)     # one type word and a parameter name
            args.append((words[0], "*" in words))
        protos[name] = (ret, args)
    return protos


def binds(decl, ct):
    """A pointer binds as c_void_p or as POINTER(the pointee's type); anything else as its own ctypes type."""
    base, pointer = decl
    if pointer:
        return ct is ctypes.c_void_p or (issubclass(ct, ctypes._Pointer) and ct._type_ is C_TYPES.get(base))
    return ct is C_TYPES[base]


def test_header_symbols_exported():
    L = ctypes.CDLL(ddsp._lib.SO_PATH)
    syms = declared_symbols()
    table = ddsp._lib.SIGNATURES
    assert set(syms) == set(ddsp._lib.EXPORTS) == set(table)
    for s in syms:
        assert hasattr(L, s), s
    # the binding's types are the header's, parameter by parameter: a wrong argtypes entry would pass garbage to a kernel
    protos = declared_prototypes()
    assert list(protos) == list(table)                  # (every declaration parsed, the table in header order)
    for name, (ret, args) in protos.items():
        restype, argtypes = table[name]
        assert restype is C_TYPES[ret], name
        assert len(argtypes) == len(args), name
        for i, (decl, ct) in enumerate(zip(args, argtypes)):
            assert binds(decl, ct), (name, i, decl, ct)


def test_abi_version_5_and_scratch_size():
    L = ddsp._lib.lib()
    assert L.ddsp_hip_abi_version() == 5 == ddsp._lib.ABI_VERSION
    assert L.ddsp_osc_scratch_bytes(0, 1, 1) == 0
    n = 64 * 500 * 100
    assert L.ddsp_osc_scratch_bytes(64, 500, 100) >= 16 * n


def test_argument_validation_without_gpu_abi5():
    L = ddsp._lib.lib()
    assert L.ddsp_osc_forward_ex(None, None, None, None, None, None, None, None, 1, 1, 1, 1, 16000, 0, None) == -1
    assert L.ddsp_osc_forward_ex(None, None, None, None, None, None, None, None, 0, 1, 1, 1, 16000, 0, None) == 0  # empty batch
    assert L.ddsp_noise_forward_ws(None, None, None, 1, 1, 65, 128, 0, 0, None, 0, None, 0, None) == -1
    assert L.ddsp_osc_set_tiling(7) == -2 and L.ddsp_osc_set_tiling(0) == 0
    # the callers' entry points validate before touching the device as well; an injected draw excludes a device counter
    # (checked first: with an empty batch the call would otherwise return 0 without a launch)
    word = ctypes.c_uint64(0)                      # (a valid address; nothing is read from it)
    p = ctypes.addressof(word)
    assert L.ddsp_noise_forward_ws(p, p, p, 0, 1, 65, 128, 0, 0, p, 0, None, 0, None) == -1
    assert L.ddsp_noise_forward_ws(p, None, p, 0, 1, 65, 128, 0, 0, p, 0, None, 0, None) == 0
    assert L.ddsp_noise_backward_ws(p, p, p, 0, 1, 65, 128, 0, 0, p, None, 0, None) == -1
    assert L.ddsp_noise_backward_ws(p, None, p, 0, 1, 65, 128, 0, 0, p, None, 0, None) == 0
    assert L.ddsp_gru_forward(None, None, None, None, None, None, None, None, None, 1, 1, 16, None) == -1
    assert L.ddsp_gru_forward(None, None, None, None, None, None, None, None, None, 0, 1, 16, None) == 0   # empty batch
    assert L.ddsp_gru_backward(None, None, None, None, None, None, None, None, None, None, None, 1, 1, 16, None) == -1
    assert L.ddsp_gru_scratch_bytes(4, 1024) == 0 and L.ddsp_gru_scratch_bytes(4, 512) > 0   # hidden sizes up to 512
    assert L.ddsp_gru_set_mode(7) == -2 and L.ddsp_gru_set_mode(0) == 0
    assert L.ddsp_spectral_loss(None, None, None, None, None, 10, 1.0, 1e-7, None) == -1
    assert L.ddsp_scaled_sigmoid_forward(None, None, 10, None) == -1 and L.ddsp_scaled_sigmoid_forward(None, None, 0, None) == 0
    assert L.ddsp_ln_lrelu_forward(None, None, None, None, None, None, 4, 512, 1e-5, 0.01, None) == -1
    assert L.ddsp_ln_lrelu_scratch_bytes(512) > 0
    assert L.ddsp_ln_lrelu_backward(None, None, None, None, None, None, None, None, None, None, None, 0, 512, 0.01, None) == -1   # empty rows still need dgamma/dbeta
    assert L.ddsp_gru_set_fault_step(-1) == -2 and L.ddsp_gru_set_fault_step(0) == 0
    # round-2 entry points: framing, one-kernel loss scale, column sums, reverb, noise backward
    assert L.ddsp_stft_frames(None, None, None, 1, 4096, 512, 128, None) == -1 and L.ddsp_stft_frames(None, None, None, 0, 4096, 512, 128, None) == 0
    assert L.ddsp_stft_frames_backward(None, None, None, 1, 4096, 512, 128, 0, None) == -1
    assert L.ddsp_mss_scale_supported(512) == 1 and L.ddsp_mss_scale_supported(96) == 0 and L.ddsp_mss_scale_supported(4096) == 0
    assert L.ddsp_mss_scale_scratch_bytes() > 0
    assert L.ddsp_mss_scale(None, None, None, None, None, None, 1, 4096, 512, 128, 1.0, 1e-7, None) == -1     # no output word
    assert L.ddsp_colsum(None, None, None, 8, 0, 0, None) == 0 and L.ddsp_colsum(None, None, None, 8, 4, 0, None) == -1
    assert L.ddsp_colsum_scratch_bytes(512) > 0 and L.ddsp_colsum_scratch_bytes(0) == 0
    assert L.ddsp_noise_backward_ws(None, None, None, 1, 1, 65, 128, 0, 0, None, None, 0, None) == -1
    assert L.ddsp_reverb_impulse(None, None, None, None, None, 16, 16, None) == -1


def test_layernorm_entry_points_validate_in_a_fixed_order():
    """The six LayerNorm + LeakyReLU entries answer, in this order: an invalid io_type; then (forward) empty rows, null pointers,
    a width the kernels are not built for -- (backward) the width, the gradient outputs an empty shard still zeroes, null pointers."""
    L = ddsp._lib.lib()
    EINVAL, ERANGE = -1, -2
    N = None
    ln_fwd = lambda rows, D: L.ddsp_ln_lrelu_forward(N, N, N, N, N, N, rows, D, 1e-5, 0.01, N)                       # noqa: E731
    ln_bwd = lambda rows, D: L.ddsp_ln_lrelu_backward(N, N, N, N, N, N, N, N, N, N, N, rows, D, 0.01, N)              # noqa: E731
    ln_fwd16 = lambda rows, D, io: L.ddsp_ln_lrelu_forward_16(N, N, N, N, N, N, rows, D, 1e-5, 0.01, io, N)          # noqa: E731
    ln_bwd16 = lambda rows, D, io: L.ddsp_ln_lrelu_backward_16(N, N, N, N, N, N, N, N, N, N, N, rows, D, 0.01, io, N)  # noqa: E731
    out_fwd = lambda rows, D, io: L.ddsp_outer_ln_lrelu_forward(N, N, N, N, N, N, N, N, rows, D, 1e-5, 0.01, io, N)  # noqa: E731
    out_bwd = lambda rows, D, io: L.ddsp_outer_ln_lrelu_backward(N, N, N, N, N, N, N, N, N, N, N, N, N, rows, D, 0.01, io, N)  # noqa: E731
    # an invalid io_type, with empty rows (which the forwards would otherwise answer with 0): the `_16` entries have no fp32 form
    for io in (0, 3, -1):
        assert ln_fwd16(0, 512, io) == EINVAL and ln_bwd16(0, 512, io) == EINVAL, io
    for io in (3, -1):
        assert out_fwd(0, 512, io) == EINVAL and out_bwd(0, 512, io) == EINVAL, io
    # empty rows with a bad width: the forward returns before it looks at D, the backward looks at D first
    for D in (0, 300, 1280):
        assert ln_fwd(0, D) == 0 and ln_fwd16(0, D, 1) == 0 and ln_fwd16(0, D, 2) == 0, D
        assert ln_bwd(0, D) == ERANGE and ln_bwd16(0, D, 1) == ERANGE and ln_bwd16(0, D, 2) == ERANGE, D
    for D in (0, 768, 1024):                               # (the first block: 256 or 512 only)
        assert all(out_fwd(0, D, io) == 0 and out_bwd(0, D, io) == ERANGE for io in (0, 1, 2)), D
    # a null grad_gamma with empty rows: an empty shard still writes its zero parameter gradients
    assert ln_bwd(0, 768) == EINVAL and ln_bwd16(0, 1024, 1) == EINVAL and ln_bwd16(0, 256, 2) == EINVAL
    assert all(out_bwd(0, D, io) == EINVAL for D in (256, 512) for io in (0, 1, 2))
    # a bad width with null pointers: the forward reports the pointers, the backward the width
    assert ln_fwd(4, 300) == EINVAL and ln_fwd16(4, 300, 1) == EINVAL and out_fwd(4, 768, 0) == EINVAL and out_fwd(4, 768, 2) == EINVAL
    assert ln_bwd(4, 300) == ERANGE and ln_bwd16(4, 300, 2) == ERANGE and out_bwd(4, 768, 0) == ERANGE and out_bwd(4, 768, 1) == ERANGE
    # negative rows, good width
    assert ln_fwd(-1, 512) == EINVAL and ln_bwd(-1, 512) == EINVAL and out_fwd(-1, 512, 0) == EINVAL and out_bwd(-1, 512, 0) == EINVAL
    # the heads and column-sum entries take all three types, and answer empty input before the type
    assert L.ddsp_heads_sigmoid_forward(N, N, N, N, 0, 1, 1, 1, 7, N) == 0 and L.ddsp_heads_sigmoid_backward(N, N, N, N, N, 0, 1, 1, 1, 7, N) == 0
    word = ctypes.c_uint64(0)                      # (a valid address; nothing is read from it)
    p = ctypes.addressof(word)
    assert L.ddsp_heads_sigmoid_forward(p, p, p, p, 1, 1, 1, 1, 7, N) == EINVAL
    assert L.ddsp_heads_sigmoid_backward(p, p, p, p, p, 1, 1, 1, 1, 7, N) == EINVAL
    assert L.ddsp_colsum(p, p, p, 8, 4, 7, N) == EINVAL and L.ddsp_colsum(N, N, N, 8, 0, 7, N) == 0


def test_module_boundary_matches_reference_contract():
    osc = ddsp.OscillatorBank(Conf(60, 16000, 128))
    sd = osc.state_dict()
    assert list(sd) == ["harmonics", "last_phases"]
    assert sd["harmonics"].dtype == torch.int64 and torch.equal(sd["harmonics"], torch.arange(1, 61))
    assert sd["last_phases"].dtype == torch.int64 and not any(p.requires_grad for p in osc.parameters())
    assert (osc.n_harmonics, osc.sample_rate, osc.hop_size) == (60, 16000, 128)
    fn = ddsp.FilteredNoise(Conf(60, 16000, 128))
    assert fn.block_size == 128 and len(fn.state_dict()) == 0
    with pytest.raises(ddsp._lib.DdspHipError):
        osc({"f0": torch.ones(1, 2, 1), "c": torch.ones(1, 2, 60), "a": torch.ones(1, 2, 1)})  # CPU tensors: no fallback
    with pytest.raises(ValueError):
        osc({"f0": torch.ones(1, 2), "c": torch.ones(1, 2, 60), "a": torch.ones(1, 2, 1)})


def test_product_path_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "ddsp-pytorch_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                text = open(os.path.join(dirpath, f)).read()
                for needle in ("import oracle", "from oracle", "libddsp_oracle", "ddsp_oracle", "oracle/"):
                    assert needle not in text, (f, needle)


def test_synthetic_controls_ranges():
    ctl = syn.make_controls(syn.CFG2, 1002, "all_live", batch=2)
    assert ctl["f0"].shape == (2, 500, 1) and ctl["c"].shape == (2, 500, 100) and ctl["H"].shape == (2, 500, 65)
    assert ctl["f0"].max() * 100 < 8000 and ctl["f0"].min() >= 39
    assert all(v.dtype == np.float32 for v in ctl.values())
    assert ctl["c"].min() >= 1e-7 and ctl["c"].max() <= 2.0 + 1e-6
    mus = syn.make_controls(syn.CFG2, 1003, "musical", batch=2)["f0"]
    assert 31.0 < mus.min() and mus.max() < 2006.0


def test_hooks_are_refused_without_opt_in():
    """The process-global *_set_* hooks change every later launch: a process that did not set DDSP_TEST_HOOKS=1 before the
    library was loaded gets DDSP_EPERM (-3) and nothing changes; restoring the default (0) is always allowed."""
    import subprocess
    import sys
    code = ("import ctypes, sys; L = ctypes.CDLL(sys.argv[1]); "
            "print(L.ddsp_test_hooks_enabled(), L.ddsp_osc_set_tiling(13), L.ddsp_osc_set_tiling(0), L.ddsp_noise_set_generic(1), "
            "L.ddsp_noise_set_generic(0), L.ddsp_gru_set_mode(2), L.ddsp_gru_set_mode(0), L.ddsp_gru_set_fault_step(3))")
    env = {k: v for k, v in os.environ.items() if k != "DDSP_TEST_HOOKS"}
    out = subprocess.run([sys.executable, "-c", code, ddsp._lib.SO_PATH], env=env, capture_output=True, text=True, check=True).stdout.split()
    assert out == ["0", "-3", "0", "-3", "0", "-3", "0", "-3"], out
    env["DDSP_TEST_HOOKS"] = "1"
    out = subprocess.run([sys.executable, "-c", code, ddsp._lib.SO_PATH], env=env, capture_output=True, text=True, check=True).stdout.split()
    assert out == ["1", "0", "0", "0", "0", "0", "0", "0"], out
    assert ddsp._lib.lib().ddsp_test_hooks_enabled() == 1          # this process: tests/conftest.py opted in
