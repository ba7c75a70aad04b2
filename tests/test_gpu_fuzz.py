"""A fixed-seed slice of the randomised parity sweep (tests/fuzz_parity.py) in the GPU suite: 150 random shapes of the
oscillator bank and the filtered noise through the C ABI against the CPU oracle -- phases bit-exact, audio <= 1e-5, noise <= 2e-6 --
plus the chunked oscillator form, the loss-side kernels, the backward of the oscillator and of the filtered noise, the filtered
noise's forward against fp64 on every kernel form, the GRU
recurrence step by step against fp64, the encoder's loudness and resampler kernels against fp64, Griffin-Lim's three kernels
one at a time against fp64, and one spectral-loss scale bin by bin against fp64."""
import pytest

pytestmark = pytest.mark.gpu

import fuzz_parity  # noqa: E402
import mss_reference  # noqa: E402


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_random_shapes_match_the_oracle(seed):
    bad, worst_audio, worst_noise = fuzz_parity.sweep(50, seed, verbose=False)
    assert bad == 0, (bad, worst_audio, worst_noise)


@pytest.mark.parametrize("seed", [21, 22])
def test_random_shapes_of_the_loss_side_kernels_match_torch(seed):
    """40 random cases per seed: one-kernel spectral-loss scales (value + gradient, any overlap), the framing pair, column sums."""
    assert fuzz_parity.sweep_training_kernels(40, seed, verbose=False) == 0


@pytest.mark.parametrize("seed", [404])
def test_random_shapes_of_the_chunked_oscillator_match_the_oracle(seed):
    bad, worst = fuzz_parity.sweep_chunked(60, seed, verbose=False)
    assert bad == 0 and worst <= 1e-5


@pytest.mark.parametrize("seed", [505])
def test_random_shapes_of_the_oscillator_backward_match_fp64(seed):
    """40 random cases of ddsp_osc_backward against the fp64 reference (tests/osc_grad_reference.py), elementwise within
    fuzz_parity.OSC_BWD_TOL of each frame's local yardstick: pinned and automatic tilings, both walks, both grad_y paths, odd f0."""
    bad, worst = fuzz_parity.sweep_osc_backward(40, seed, verbose=False)
    assert bad == 0, (bad, worst)


@pytest.mark.parametrize("seed", [606])
def test_random_shapes_of_the_noise_backward_match_fp64(seed):
    """40 random cases of ddsp_noise_backward_ws against the fp64 reference (tests/noise_grad_reference.py), elementwise within
    fuzz_parity.NOISE_BWD_TOL of each frame's yardstick: every kernel form, injected and in-kernel draws, forced modes, zero frames."""
    bad, worst = fuzz_parity.sweep_noise_backward(40, seed, verbose=False)
    assert bad == 0, (bad, worst)


@pytest.mark.parametrize("seed", [616])
def test_random_shapes_of_the_noise_forward_match_fp64(seed):
    """40 random cases of ddsp_noise_forward_ws against the fp64 reference (tests/noise_fwd_reference.py): the direct forms per sample
    within TOL_SAMPLE of Y[n], every form per frame within TOL_FRAME of Yframe and 2e-6 of the frame's own
    peak: every kernel form, injected and in-kernel draws, forced modes and lane counts, frame levels over seven decades, zero frames.

    (With single fp32 chains the frame kernel missed the peak contract here at 26 bands / hop 5, 2.4e-6, and the batched kernel at
    973 and 426 bands / hop 1024, 3.1e-6 and 2.2e-6: DESIGN.md section 5 has what changed in csrc/ddsp_noise.hip.)"""
    bad, worst = fuzz_parity.sweep_noise_forward(40, seed, verbose=False)
    print(f"noise forward sweep seed {seed}: " + ", ".join(f"{k} {v:.1e}" for k, v in sorted(worst.items())))
    assert bad == 0, (bad, worst)


@pytest.mark.parametrize("seed", [707])
def test_random_shapes_of_the_gru_recurrence_match_fp64_step_by_step(seed):
    """40 random cases of the GRU recurrence's raw launchers against the teacher-forced fp64 reference (tests/gru_reference.py), every
    tensor within 8 x the same formulas' fp32 error: fp32 and bf16 kernels, with and without h0 / bias / dhT, 16-bit gradient outputs.
    The seed reaches both bf16 matrix-core kernels at all four KP."""
    counts = {}
    bad, worst = fuzz_parity.sweep_gru(40, seed, verbose=False, counts=counts)
    assert bad == 0, (bad, worst)
    assert {f"gru_{d}_mfma_kernel<{KP}>" for d in ("fwd", "bwd") for KP in (4, 8, 16, 32)} <= set(counts), counts


@pytest.mark.parametrize("seed", [808])
def test_random_cases_of_the_encoder_stages_match_fp64(seed):
    """40 random cases, alternately ddsp_loudness (random n_fft, hop and frame count, every hop-long segment at its own level over six
    decades or exactly zero) and ddsp_resample (random rate pair, L <= 20 000), against the fp64 references of
    tests/encoder_reference.py: loudness 2e-6, resampled audio 1e-6 (tests/test_encoder_reference_host.py holds the stock fp32
    branch to half of that on the same cases)."""
    bad, worst = fuzz_parity.sweep_encoder_stages(40, seed, verbose=False)
    assert bad == 0, (bad, worst)


@pytest.mark.parametrize("seed", [909])
def test_random_cases_of_the_griffinlim_stages_match_fp64(seed):
    """40 random cases of Griffin-Lim's synthesis, overlap-add and analysis kernels, each alone through ddsp_griffinlim_stage, under
    the criteria of tests/griffinlim_reference.py: the transforms at most CPU_FACTOR times the CPU fp32 formulation's error and
    under the derived ceiling, the overlap-add bit for bit its fp32 restatement and within the summation bound."""
    bad, report = fuzz_parity.sweep_griffinlim_stages(40, seed, verbose=False)
    assert bad == 0, (bad, report)



@pytest.mark.parametrize("seed", mss_reference.SWEEP_SEEDS)
def test_random_cases_of_one_spectral_loss_scale_match_fp64_bin_by_bin(seed):
    """30 random cases of ddsp_mss_scale called directly (random n_fft, hop 1 .. n_fft, B, L, alpha, eps, segment levels) under the
    criteria of tests/mss_reference.py: every bin of the gradient spectrum within its derived bound or CPU_FACTOR times the stock
    fp32 formulation's error, undecided bins against the candidate signs and under their cap, lin and log each within 2e-5."""
    bad, worst = fuzz_parity.sweep_mss_stages(mss_reference.SWEEP_CASES, seed, verbose=False)
    print(f"MSS sweep seed {seed}: worst error / bound {worst:.4f}")
    assert bad == 0 and worst <= 1.0, (bad, worst)
