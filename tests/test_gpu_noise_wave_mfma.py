"""noise_forward at hop 128 / 65 bands -- the wavefront-private kernel whose truncated convolution runs on the matrix cores as 4 x 4
fp32 outer products (csrc/ddsp_noise_wave.hip, csrc/ddsp_noise_conv_plan.h) -- against oracle/torch_restatement.filtered_noise,
evaluated in fp64 on the same filter magnitudes and the same draw, with the 2e-6 criterion of tests/test_gpu_parity.py.

Frame counts: 16 (one group), 48 (the first, a middle and the last group of one wavefront's software pipeline when the grid is one
wavefront, and three wavefronts otherwise), 17 and 31 (a remainder that goes to the batched kernel), and 35 008 (2 188 groups: more
than eight per CU, so that the residency knob decides the grid and every wavefront walks several groups).  Overwriting and accumulating,
injected draw and in-kernel Philox; residency 1, 4 and 8 must give the same bits."""
import numpy as np
import pytest
import torch

import ddsp_pytorch_amd as ddsp
from ddsp_pytorch_amd import synthetic as syn
from oracle import oracle
from oracle import torch_restatement as tr

pytestmark = pytest.mark.gpu
TOL = 2e-6
HOP, NF = 128, 65
SEED, OFFSET = 31337, (5 << 32) + 77


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def case(B, T, injected):
    """-> (H [B, T, 65] fp32, the injected draw or None, the fp64 reference [B, T * 128])"""
    rng = np.random.default_rng(1000 * B + T + int(injected))
    H = syn.controller_range(rng.standard_normal((B, T, NF), dtype=np.float32))
    u = rng.random((B, T, HOP), dtype=np.float32) if injected else None
    draw = u if injected else oracle.philox_uniform(SEED, OFFSET, B, T, HOP)
    ref = tr.filtered_noise(torch.from_numpy(H).double(), HOP, uniform=torch.from_numpy(draw).double()).numpy()
    return H, u, ref


def run_all_residencies(fn):
    L = ddsp._lib.lib()
    outs = []
    try:
        for level in (4, 1, 8):
            assert L.ddsp_noise_set_residency(level) == 0
            outs.append(fn())
    finally:
        L.ddsp_noise_set_residency(0)
    for y in outs[1:]:
        assert torch.equal(y, outs[0])
    return outs[0]


@pytest.mark.parametrize("injected", [True, False])
@pytest.mark.parametrize("B,T", [(1, 16), (1, 48), (1, 17), (1, 31), (3, 16), (547, 64)])
def test_against_the_reference_overwrite_and_accumulate_at_every_residency(B, T, injected):
    H, u, ref = case(B, T, injected)
    kw = dict(uniform=dev(u)) if injected else dict(seed=SEED, offset=OFFSET)
    Hd = dev(H)
    y = run_all_residencies(lambda: ddsp.noise_forward(Hd, HOP, **kw))
    err = float(np.max(np.abs(y.cpu().numpy() - ref)))
    print(f"B {B} T {T} injected {injected}: max |y - ref| = {err:.3e}")
    assert err <= TOL
    base = torch.from_numpy(np.random.default_rng(T).standard_normal((B, T * HOP)).astype(np.float32)).cuda()
    acc = run_all_residencies(lambda: ddsp.noise_forward(Hd, HOP, out=base.clone(), accumulate=True, **kw))
    # accumulating adds the same fp32 value to what was there: one rounding of base + y, the very one torch makes
    assert torch.equal(acc, base + y)
