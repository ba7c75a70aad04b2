"""ddsp_mfcc on the device against the fp64 restatement (tests/mfcc_reference.py), element by element, coefficients and log-mel:
every transform size, odd frame counts and a single frame, hops below, at and unrelated to the frame length, band counts from 8
to 128 (128 bands on 33 bins included), and the structural promises -- a row's bits do not depend on the batch, a second run
repeats them, nothing is written behind the outputs, the grid-stride loop past the block cap, a captured graph.

The tolerance is KERNEL_FACTOR x C_CPU times each element's own bound; both constants come from the CPU evaluation (see the
reference's docstring), not from the kernel."""
import os
import sys

import numpy as np
import pytest
import torch

import ddsp_pytorch_amd as ddsp
from ddsp_pytorch_amd import encoder as enc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mfcc_reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu

C_KERNEL = ref.KERNEL_FACTOR * ref.C_CPU
LOG_FLOOR = np.float32(np.log(np.float64(np.float32(ref.FLOOR))))        # fl32(log(floor))


def run(x, n_fft, hop, n_mels, n_mfcc, logmel=True):
    out = ddsp.mfcc(torch.from_numpy(x).cuda(), n_fft, hop, ref.SAMPLE_RATE, n_mels=n_mels, n_mfcc=n_mfcc, return_logmel=logmel)
    torch.cuda.synchronize()
    return (out[0].cpu().numpy(), out[1].cpu().numpy()) if logmel else (out.cpu().numpy(), None)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("n_fft", ref.N_FFTS)
def test_kernel_against_fp64(n_fft):
    worst = (0.0, None)
    for name, x, n, hop, pairs in ref.cases():
        if n != n_fft:
            continue
        spec = ref.spectrum(x, n_fft, hop)
        for n_mels, n_mfcc in pairs:
            want = ref.from_spectrum(spec, n_fft, ref.SAMPLE_RATE, n_mels, n_mfcc)
            got, lm = run(x, n_fft, hop, n_mels, n_mfcc)
            r, where = ref.worst_ratio(got, lm, want)      # (asserts the NaN frames, and that no other frame holds a NaN)
            if r > worst[0]:
                worst = (r, (name, n_mels, n_mfcc, where))
            if name.startswith("zero_beside_loud"):
                # the all-zero frames: every band is exactly fl32(log(floor))
                for b, f in ((0, 1), (1, 0), (1, 2)):
                    assert np.array_equal(bits(lm[b, f]), bits(np.full(n_mels, LOG_FLOOR))), (name, b, f)
            if name.startswith("non_finite"):
                assert want["dead"].tolist() == [[True, False, False], [False, False, True]]
    print(f"n_fft {n_fft}: worst |error| / bound(c = 1) = {worst[0]:.3f} at {worst[1]} (allowed {C_KERNEL})")
    assert worst[0] <= C_KERNEL, worst


@pytest.mark.parametrize("n_fft", ref.N_FFTS)
def test_rows_alone_a_second_run_and_a_null_logmel_give_the_same_bits(n_fft):
    rng = np.random.default_rng(n_fft)
    hop = n_fft // 4
    x = rng.uniform(-1, 1, (3, n_fft + 4 * hop + 1)).astype(np.float32)        # 5 frames: the last pair is half empty
    x[1] *= 1e-3
    got, lm = run(x, n_fft, hop, 40, 13)
    again, lm_again = run(x, n_fft, hop, 40, 13)
    assert np.array_equal(bits(got), bits(again)) and np.array_equal(bits(lm), bits(lm_again))
    for b in range(3):
        alone, lm_alone = run(x[b:b + 1], n_fft, hop, 40, 13)
        assert np.array_equal(bits(alone[0]), bits(got[b])) and np.array_equal(bits(lm_alone[0]), bits(lm[b])), b
    only, _ = run(x, n_fft, hop, 40, 13, logmel=False)
    assert np.array_equal(bits(only), bits(got))


@pytest.mark.parametrize("n_fft,F", [(64, 5), (512, 3), (1024, 1), (2048, 2)])
def test_nothing_is_written_behind_the_outputs(n_fft, F):
    n_mels, n_mfcc, hop, B, guard = 40, 13, 3, 2, 4096
    x = torch.from_numpy(ref.noise_input(n_fft, F, hop)).cuda()
    t = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in enc.mfcc_tables(n_fft, ref.SAMPLE_RATE, n_mels, n_mfcc).items()}
    n_out, n_lm = B * F * n_mfcc, B * F * n_mels
    out = torch.full((guard + n_out + guard,), -7.0, device="cuda")
    lm = torch.full((guard + n_lm + guard,), -7.0, device="cuda")
    rc = ddsp._lib.lib().ddsp_mfcc(x.data_ptr(), t["band_start"].data_ptr(), t["band_count"].data_ptr(), t["band_w"].data_ptr(),
                                   t["dct"].data_ptr(), out[guard:].data_ptr(), lm[guard:].data_ptr(), B, x.shape[1], n_fft, hop,
                                   n_mels, n_mfcc, t["scale"], ref.FLOOR, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0
    for buf, n in ((out, n_out), (lm, n_lm)):
        assert bool((buf[:guard] == -7.0).all()) and bool((buf[guard + n:] == -7.0).all())
        assert bool(torch.isfinite(buf[guard:guard + n]).all()) and not bool((buf[guard:guard + n] == -7.0).any())
    want, want_lm = ddsp.mfcc(x, n_fft, hop, ref.SAMPLE_RATE, n_mels=n_mels, n_mfcc=n_mfcc, return_logmel=True)
    assert torch.equal(out[guard:guard + n_out].view_as(want), want) and torch.equal(lm[guard:guard + n_lm].view_as(want_lm), want_lm)


def test_more_units_than_the_block_cap():
    """n_fft 64, hop 16, one row of 2.1 M samples: 8 203 units for at most 8 192 blocks, so some blocks take a second unit."""
    x = ref.big_case()
    b = ref.BIG
    F = (x.shape[1] - b["n_fft"]) // b["hop"] + 1
    assert ((F + 1) // 2 + 7) // 8 > 8192
    got, lm = run(x, b["n_fft"], b["hop"], b["n_mels"], b["n_mfcc"])
    want = ref.big_reference(x)
    r, where = ref.worst_ratio(got, lm, want)
    print(f"long row: worst |error| / bound(c = 1) = {r:.3f} at {where} (allowed {C_KERNEL})")
    assert r <= C_KERNEL, (r, where)
    zero = np.flatnonzero(np.all(lm[0] == LOG_FLOOR, axis=-1))
    assert zero.size >= (400 - 64) // 16                     # the all-zero stretch


def test_captured_graph_replays_on_changed_input():
    n_fft, hop = 2048, 512
    x = torch.from_numpy(ref.noise_input(n_fft, 5, hop)).cuda()
    static = x.clone()
    ddsp.mfcc(static, n_fft, hop, ref.SAMPLE_RATE, return_logmel=True)         # tables to the device outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, lm = ddsp.mfcc(static, n_fft, hop, ref.SAMPLE_RATE, return_logmel=True)
    for scale in (1.0, 0.25):
        static.copy_(x * scale)
        graph.replay()
        torch.cuda.synchronize()
        want, want_lm = ddsp.mfcc(x * scale, n_fft, hop, ref.SAMPLE_RATE, return_logmel=True)
        assert torch.equal(out, want) and torch.equal(lm, want_lm), scale
    assert not torch.equal(want, ddsp.mfcc(x, n_fft, hop, ref.SAMPLE_RATE))
