"""ctypes binding of libddsp_hip.so (C ABI in include/ddsp_hip.h).

There is deliberately no fallback: if the HIP library is missing or a launch
fails, the caller gets an exception -- never a silent PyTorch/CPU path.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

_DIR = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("DDSP_HIP_LIB", os.path.join(_DIR, "libddsp_hip.so"))  # override: A/B builds (tools/ab_bench.sh)
ABI_VERSION = 5

_lib = None


class DdspHipError(RuntimeError):
    pass


def build(force: bool = False, jobs: int = 4) -> str:
    """Compile csrc/*.hip for gfx950 into libddsp_hip.so (hipcc cross-compiles without a GPU)."""
    args = ["make", "-C", os.path.join(_DIR, "csrc"), f"-j{jobs}"]
    if force:
        args.append("-B")
    r = subprocess.run(args, capture_output=True, text=True)
    if r.returncode != 0:
        raise DdspHipError("building libddsp_hip.so failed:\n" + r.stdout[-4000:] + r.stderr[-4000:])
    return SO_PATH


_vp, _i32, _u32, _u64, _long, _size, _f32, _f64 = (ctypes.c_void_p, ctypes.c_int, ctypes.c_uint, ctypes.c_uint64, ctypes.c_long,
                                                   ctypes.c_size_t, ctypes.c_float, ctypes.c_double)

# The binding of every symbol include/ddsp_hip.h declares, in the header's order: name -> (restype, argtypes).
# tests/test_host_abi.py checks it against the header's prototypes.
SIGNATURES = {
    "ddsp_hip_abi_version": (_i32, []),
    "ddsp_test_hooks_enabled": (_i32, []),
    "ddsp_osc_scratch_bytes": (_size, [_i32, _i32, _i32]),
    "ddsp_osc_forward_ex": (_i32, [_vp] * 8 + [_i32] * 5 + [_u32, _vp]),
    "ddsp_noise_workspace_bytes": (_size, [_i32, _i32, _i32, _i32]),
    "ddsp_noise_forward_ws": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _u64, _u64, _vp, _i32, _vp, _size, _vp]),
    "ddsp_noise_backward_ws": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _u64, _u64, _vp, _vp, _size, _vp]),
    "ddsp_noise_ola_workspace_bytes": (_size, [_i32, _i32, _i32, _i32]),
    "ddsp_noise_ola_forward": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _u64, _u64, _vp, _i32, _vp, _size, _vp]),
    "ddsp_noise_ola_backward": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _u64, _u64, _vp, _vp, _size, _vp]),
    "ddsp_noise_ola_stream_state_floats": (_size, [_i32]),
    "ddsp_noise_ola_stream": (_i32, [_vp] * 6 + [_i32, _i32, _i32, _i32, _u64, _u64, _vp, _vp, _size, _vp]),
    "ddsp_osc_backward_scratch_bytes": (_size, [_i32, _i32, _i32]),
    "ddsp_osc_backward": (_i32, [_vp] * 8 + [_i32] * 5 + [_vp]),
    "ddsp_osc_set_tiling": (_i32, [_i32]),
    "ddsp_osc_set_path": (_i32, [_i32]),
    "ddsp_osc_plan": (_i32, [_i32] * 5 + [ctypes.POINTER(_i32), _i32]),
    "ddsp_osc_clock": (_i32, [_vp, _i32, _i32, _i32, _i32, _i32, ctypes.POINTER(ctypes.c_double), _vp]),
    "ddsp_noise_set_residency": (_i32, [_i32]),
    "ddsp_noise_get_residency": (_i32, []),
    "ddsp_noise_conv_probe": (_i32, [_vp, _vp, _vp, _vp]),
    "ddsp_noise_set_generic": (_i32, [_i32]),
    "ddsp_profile_enable": (_i32, [_i32]),
    "ddsp_profile_select": (_i32, [_u32]),
    "ddsp_profile_read": (_i32, [ctypes.POINTER(_i32), ctypes.POINTER(_f32), _i32]),
    "ddsp_gru_scratch_bytes": (_size, [_i32, _i32]),
    "ddsp_gru_max_batch": (_i32, [_i32, _i32]),
    "ddsp_gru_forward": (_i32, [_vp] * 9 + [_i32] * 3 + [_vp]),
    "ddsp_gru_backward": (_i32, [_vp] * 11 + [_i32] * 3 + [_vp]),
    "ddsp_gru_status": (_i32, [_vp, ctypes.POINTER(_i32)]),
    "ddsp_gru_forward_bf16": (_i32, [_vp] * 9 + [_i32] * 3 + [_vp]),
    "ddsp_gru_backward_bf16": (_i32, [_vp] * 11 + [_i32] * 4 + [_vp]),
    "ddsp_gru_set_mode": (_i32, [_i32]),
    "ddsp_gru_set_fault_step": (_i32, [_i32]),
    "ddsp_outer_ln_lrelu_scratch_bytes": (_size, [_i32]),
    "ddsp_outer_ln_lrelu_forward": (_i32, [_vp] * 8 + [_long, _i32, _f32, _f32, _i32, _vp]),
    "ddsp_outer_ln_lrelu_backward": (_i32, [_vp] * 13 + [_long, _i32, _f32, _i32, _vp]),
    "ddsp_colsum_scratch_bytes": (_size, [_i32]),
    "ddsp_colsum": (_i32, [_vp, _vp, _vp, _long, _i32, _i32, _vp]),
    "ddsp_stft_frames": (_i32, [_vp, _vp, _vp, _long, _long, _i32, _i32, _vp]),
    "ddsp_stft_frames_backward": (_i32, [_vp, _vp, _vp, _long, _long, _i32, _i32, _i32, _vp]),
    "ddsp_mss_scale_scratch_bytes": (_size, []),
    "ddsp_mss_scale_supported": (_i32, [_i32]),
    "ddsp_mss_scale": (_i32, [_vp] * 6 + [_long, _long, _i32, _i32, _f32, _f32, _vp]),
    "ddsp_reverb_impulse": (_i32, [_vp] * 5 + [_i32, _i32, _vp]),
    "ddsp_reverb_impulse_backward": (_i32, [_vp] * 8 + [_i32, _i32, _vp]),
    "ddsp_spectral_mul": (_i32, [_vp, _vp, _vp, _long, _long, _vp]),
    "ddsp_spectral_mul_backward": (_i32, [_vp] * 5 + [_long, _long, _vp]),
    "ddsp_reverb_live_scratch_bytes": (_size, [_i32, _i32]),
    "ddsp_reverb_live": (_i32, [_vp] * 9 + [_i32, _i32, _vp]),
    "ddsp_spectral_loss_scratch_bytes": (_size, []),
    "ddsp_spectral_loss": (_i32, [_vp] * 5 + [_long, _f32, _f32, _vp]),
    "ddsp_scaled_sigmoid_forward": (_i32, [_vp, _vp, _long, _vp]),
    "ddsp_scaled_sigmoid_backward": (_i32, [_vp, _vp, _vp, _long, _vp]),
    "ddsp_heads_sigmoid_forward": (_i32, [_vp] * 4 + [_long, _i32, _i32, _i32, _i32, _vp]),
    "ddsp_heads_sigmoid_backward": (_i32, [_vp] * 5 + [_long, _i32, _i32, _i32, _i32, _vp]),
    "ddsp_ln_lrelu_scratch_bytes": (_size, [_i32]),
    "ddsp_ln_lrelu_forward": (_i32, [_vp] * 6 + [_long, _i32, _f32, _f32, _vp]),
    "ddsp_ln_lrelu_backward": (_i32, [_vp] * 11 + [_long, _i32, _f32, _vp]),
    "ddsp_ln_lrelu_forward_16": (_i32, [_vp] * 6 + [_long, _i32, _f32, _f32, _i32, _vp]),
    "ddsp_ln_lrelu_backward_16": (_i32, [_vp] * 11 + [_long, _i32, _f32, _i32, _vp]),
    "ddsp_resample": (_i32, [_vp] * 4 + [_long, _long, _i32, _i32, _i32, _vp]),
    "ddsp_crepe_frames": (_i32, [_vp] * 3 + [_long, _long, _i32, _long, _vp]),
    "ddsp_crepe_epilogue": (_i32, [_vp] * 7 + [_long, _i32, _i32, _i32, _vp]),
    "ddsp_pitch_decode": (_i32, [_vp] * 8 + [_long, _vp]),
    "ddsp_pitch_centered": (_i32, [_vp] * 6 + [_long, _vp]),
    "ddsp_pitch_viterbi_workspace_bytes": (_size, [_long, _long]),
    "ddsp_pitch_viterbi": (_i32, [_vp] * 6 + [_long, _long, _vp]),
    "ddsp_pitch_voicing_workspace_bytes": (_size, [_long, _long]),
    "ddsp_pitch_voicing": (_i32, [_vp] * 11 + [_long, _long, _i32, _i32, _f32, _f32, _f32, _i32, _vp]),
    "ddsp_condition_accum_bytes": (_size, [_long, _i32]),
    "ddsp_condition_launch_shape": (_i32, [_i32, _long, _long, ctypes.POINTER(_i32), ctypes.POINTER(_long)]),
    "ddsp_condition_stats": (_i32, [_vp] * 5 + [_long, _long, _i32, _i32, _f32, _f32, _f32, _f32, _vp]),
    "ddsp_condition_tables": (_i32, [_vp] * 5 + [_long, _i32, _i32, _f32, _f32, _vp]),
    "ddsp_condition_apply": (_i32, [_vp] * 14 + [_long] * 4 + [_i32] * 4 + [_f32, _long, _vp]),
    "ddsp_tuning_accum_bytes": (_size, [_long]),
    "ddsp_tuning_stats": (_i32, [_vp] * 5 + [_long, _long, _i32, _f32, _f32, _vp]),
    "ddsp_tuning_estimate": (_i32, [_vp] * 5 + [_long, _i32, _i32, _vp]),
    "ddsp_tuning_workspace_bytes": (_size, [_long, _long]),
    "ddsp_tuning_apply": (_i32, [_vp] * 13 + [_long, _long, _long, _i32, _i32, _long, _long, _long, _i32, _f32, _f32, _f32, _vp]),
    "ddsp_yin_salience": (_i32, [_vp] * 3 + [_long, _long, _i32, _long, _vp]),
    "ddsp_harm_workspace_bytes": (_size, [_long, _long, _i32]),
    "ddsp_harm_analysis": (_i32, [_vp] * 7 + [_long, _long, _i32, _i32, _i32, _i32, _vp]),
    "ddsp_harm_resynth": (_i32, [_vp] * 6 + [_long, _long, _i32, _i32, _i32, _u32, _vp]),
    "ddsp_harm_refine_workspace_bytes": (_size, [_long, _long, _i32]),
    "ddsp_harm_refine": (_i32, [_vp] * 8 + [_long, _long, _i32, _i32, _i32, _i32, _f32, _u32, _vp]),
    "ddsp_noise_analysis_workspace_bytes": (_size, [_long, _long, _i32, _i32]),
    "ddsp_noise_analysis": (_i32, [_vp] * 4 + [_long, _long, _i32, _i32, _i32, _i32, _vp]),
    "ddsp_noise_analysis_ola_workspace_bytes": (_size, [_long, _long, _i32, _i32]),
    "ddsp_noise_analysis_ola": (_i32, [_vp] * 4 + [_long, _long, _i32, _i32, _i32, _i32, _vp]),
    "ddsp_transform_controls": (_i32, [_vp] * 11 + [_long, _long, _long, _i32, _i32, _i32, _i32, _vp]),
    "ddsp_morph_controls": (_i32, [_vp] * 17 + [_long, _long, _long, _long, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "ddsp_dtw_workspace_bytes": (_size, [_long, _long, _long]),
    "ddsp_dtw_align": (_i32, [_vp] * 8 + [_size, _long, _long, _long, _i32, _long, _long, _f32, _f64, _vp]),
    "ddsp_loudness_supported": (_i32, [_i32]),
    "ddsp_loudness": (_i32, [_vp] * 3 + [_long, _long, _i32, _i32, _vp]),
    "ddsp_mfcc": (_i32, [_vp] * 7 + [_long, _long, _i32, _i32, _i32, _i32, _f32, _f32, _vp]),
    "ddsp_voices_allocate": (_i32, [_vp] * 16 + [_long, _long, _i32, _long, _i32, _i32, _long, _vp]),
    "ddsp_voices_mix": (_i32, [_vp] * 4 + [_long, _i32, _i32, _long, _long, _long, _long, _long, _vp]),
    "ddsp_wavetable_supported": (_i32, [_i32, _i32]),
    "ddsp_wavetable_form": (_i32, [_i32] * 5),
    "ddsp_wavetable_scratch_bytes": (_size, [_i32] * 5),
    "ddsp_wavetable_forward": (_i32, [_vp] * 7 + [_i32] * 6 + [_vp]),
    "ddsp_wavetable_backward_scratch_bytes": (_size, [_i32] * 5),
    "ddsp_wavetable_backward": (_i32, [_vp] * 10 + [_i32] * 6 + [_vp]),
    "ddsp_wavetable_set_form": (_i32, [_i32]),
    "ddsp_wavetable_set_grid": (_i32, [_i32]),
    "ddsp_wavetable_mip_levels": (_i32, [_i32]),
    "ddsp_wavetable_mip_build": (_i32, [_vp] * 3 + [_i32, _i32, _vp]),
    "ddsp_wavetable_mip_adjoint": (_i32, [_vp] * 3 + [_i32, _i32, _vp]),
    "ddsp_wavetable_form_bl": (_i32, [_i32] * 5),
    "ddsp_wavetable_forward_bl": (_i32, [_vp] * 6 + [_i32] * 6 + [_vp]),
    "ddsp_wavetable_backward_bl_scratch_bytes": (_size, [_i32] * 5),
    "ddsp_wavetable_backward_bl": (_i32, [_vp] * 10 + [_i32] * 6 + [_vp]),
    "ddsp_wavetable_set_mip_lds": (_i32, [_long]),
    "ddsp_sinusoids_supported": (_i32, [_i32, _i32]),
    "ddsp_sinusoids_scratch_bytes": (_size, [_i32] * 4),
    "ddsp_sinusoids_forward": (_i32, [_vp] * 6 + [_i32] * 6 + [_vp]),
    "ddsp_sinusoids_backward_scratch_bytes": (_size, [_i32] * 5),
    "ddsp_sinusoids_backward": (_i32, [_vp] * 9 + [_i32] * 6 + [_vp]),
    "ddsp_sinusoids_set_form": (_i32, [_i32]),
    "ddsp_sinusoids_set_grid": (_i32, [_i32]),
    "ddsp_partials_supported": (_i32, [_i32, _i32, _i32]),
    "ddsp_partials_workspace_bytes": (_size, [_long, _long, _i32, _i32, _i32]),
    "ddsp_partials_analysis": (_i32, [_vp] * 8 + [_long, _long, _i32, _i32, _i32, _i32, _vp]),
    "ddsp_partials_resynth": (_i32, [_vp] * 6 + [_long, _long, _i32, _i32, _i32, _u32, _vp]),
    "ddsp_pcm_to_mono": (_i32, [_vp, _vp, _long, _i32, _i32, _vp]),
    "ddsp_make_examples": (_i32, [_vp, _long, _vp, _i32, _long, _long, _long, _long, _i32, _vp, _vp, _vp]),
    "ddsp_griffinlim_supported": (_i32, [_i32]),
    "ddsp_griffinlim_workspace_bytes": (_size, [_long, _long, _i32, _i32]),
    "ddsp_griffinlim": (_i32, [_vp] * 6 + [_size, _long, _long, _i32, _i32, _long, _i32, _f32, _vp]),
    "ddsp_wfft_probe_sizes": (_i32, [_i32, _long, ctypes.POINTER(_long), ctypes.POINTER(_long)]),
    "ddsp_wfft_probe": (_i32, [_i32, _vp, _vp, _long, _vp]),
    "ddsp_notes_expression": (_i32, [_vp] * 9 + [_long, _long, _long, _long, _vp]),
    "ddsp_notes_render_expr": (_i32, [_vp] * 14 + [_long, _long, _long, _long, _i32] + [_long] * 6 + [_f64, _f64, _f32, _f32] + [_vp] * 7 +
                               [_long, _long, _f64, _f64, _long, _long, _vp]),
    "ddsp_griffinlim_stage": (_i32, [_i32] + [_vp] * 8 + [_long, _long, _i32, _i32, _long, _f32, _vp]),
    "ddsp_notes_extract": (_i32, [_vp] * 12 + [_long, _long, _long, _long, _i32, _i32, _long, _long, _i32, _f32, _f32, _vp]),
    "ddsp_notes_render": (_i32, [_vp] * 14 + [_long, _long, _long, _long, _i32] + [_long] * 6 + [_f64, _f64, _f32, _f32, _vp]),
    "ddsp_gather_batch": (_i32, [_vp, _vp, ctypes.POINTER(_long), _i32, _vp, _vp, _long, _long, _i32, _i32, _vp, _vp]),
}
EXPORTS = tuple(SIGNATURES)


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise DdspHipError(
            f"{SO_PATH} is missing: the DDSP hot path has no CPU fallback. "
            "Build it with `python -c 'import __graft_entry__ as g; g.build()'` or `make -C ddsp-pytorch_amd/csrc`.")
    L = ctypes.CDLL(SO_PATH)
    # first of all: a stale library (it is git-ignored and not rebuilt on import) must say "rebuild", not fail on a missing symbol
    abi = L.ddsp_hip_abi_version()          # (ctypes' default binding: int, no arguments)
    if abi != ABI_VERSION:
        raise DdspHipError(f"{SO_PATH} has ABI {abi}, expected {ABI_VERSION}: rebuild "
                           "(`make -C ddsp-pytorch_amd/csrc` or __graft_entry__.build())")
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


KERNEL_NAMES = {1: "osc_frame_totals", 2: "osc_scan", 3: "osc_frame_synth", 4: "noise_frame", 5: "noise_impulse_responses"}


def profile_enable(capacity: int, only=None) -> None:
    """`only`: kernel names (KERNEL_NAMES values) to record; None = every kernel."""
    mask = 0
    for name in only or ():
        mask |= 1 << [k for k, v in KERNEL_NAMES.items() if v == name][0]
    check(lib().ddsp_profile_select(mask), "ddsp_profile_select")
    check(lib().ddsp_profile_enable(capacity), "ddsp_profile_enable")


def profile_read(cap: int = 65536):
    """-> list of (kernel name, milliseconds) recorded since the last read."""
    ids = (ctypes.c_int * cap)()
    ms = (ctypes.c_float * cap)()
    n = lib().ddsp_profile_read(ids, ms, cap)
    return [(KERNEL_NAMES.get(ids[i], str(ids[i])), float(ms[i])) for i in range(n)]


def check(rc: int, what: str) -> None:
    if rc == 0:
        return
    if rc == -1:
        raise DdspHipError(f"{what}: invalid argument (DDSP_EINVAL)")
    if rc == -2:
        raise DdspHipError(f"{what}: shape outside the supported range (DDSP_ERANGE)")
    if rc == -3:
        raise DdspHipError(f"{what}: test / tuning hook refused (DDSP_EPERM): set DDSP_TEST_HOOKS=1 before the library is loaded")
    raise DdspHipError(f"{what}: HIP error {rc}")


def osc_plan(B: int, T: int, H: int, hop: int, sample_rate: int) -> dict:
    """What ddsp_osc_forward_ex (flags 0) launches for this shape on the current device (include/ddsp_hip.h: ddsp_osc_plan)."""
    out = (ctypes.c_int * 8)()
    check(lib().ddsp_osc_plan(B, T, H, hop, sample_rate, out, 8), "ddsp_osc_plan")
    keys = ("harmonics_per_lane", "lanes_per_row", "chunked", "chunk_samples", "chunks_per_row", "row_blocks",
            "compute_units", "workgroups_per_unit")
    return dict(zip(keys, list(out)))


def osc_clock(scratch, B: int, T: int, H: int, hop: int, sample_rate: int, stream: int = 0) -> float:
    """Shader clock (GHz) of the synth kernel of the last ddsp_osc_forward_ex on `scratch` (a torch uint8 tensor); synchronises."""
    ghz = ctypes.c_double(0.0)
    check(lib().ddsp_osc_clock(scratch.data_ptr(), B, T, H, hop, sample_rate, ctypes.byref(ghz), stream or None), "ddsp_osc_clock")
    return float(ghz.value)
