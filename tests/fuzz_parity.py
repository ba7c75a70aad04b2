#!/usr/bin/env python3
"""Randomised parity sweep of the HIP path against the CPU oracle (the test_*.py files hold the fixed cases; this is the wide
net, run by tests/test_gpu_fuzz.py with a fixed seed and from the command line for bigger sweeps):
random batch / frames / harmonics / hop / sample rate / noise bands, both f0 kinds, power-of-two and odd hops, hops 256 / 512
(in-LDS FFT noise form, impulse shorter than / equal to / longer than the hop), the benchmarked noise forms with ragged frame
counts, the in-kernel draw, and -- in a third of the cases -- loudness / filter levels spread over seven decades from frame to
frame.  Prints one line per case and a summary; exit code 1 if any case exceeds the tolerances the tests assert, taken LOCALLY:
audio 1e-5 of the loudness around each sample, noise 2e-6 of each frame's own level (or peak), phases bit-exact.
usage: fuzz_parity.py [cases] [seed] [training | chunked | backward | noise_backward | noise_forward | gru | encoder | griffinlim | mss]   (`training`: the loss-side kernels against
fp64 torch instead; `chunked`: the chunked oscillator form with forced tilings and chunk lengths; `backward`: the oscillator's
backward against the fp64 reference of tests/osc_grad_reference.py; `noise_backward`: the filtered noise's backward against the
fp64 reference of tests/noise_grad_reference.py; `noise_forward`: the filtered noise's forward, every kernel form, against the fp64
reference and yardsticks of tests/noise_fwd_reference.py; `gru`: the GRU recurrence, fp32 and bf16 kernels, step by step against the fp64
reference of tests/gru_reference.py; `encoder`: the encoder's loudness and resampler kernels against the fp64 references of
tests/encoder_reference.py; `griffinlim`: Griffin-Lim's synthesis, overlap-add and analysis kernels one at a time through
ddsp_griffinlim_stage against the fp64 reference and the criteria of tests/griffinlim_reference.py; `mss`: one spectral-loss
scale through ddsp_mss_scale, every bin of its gradient spectrum against the fp64 reference and bounds of tests/mss_reference.py)"""
import os
import sys

import numpy as np
import torch

os.environ.setdefault("DDSP_TEST_HOOKS", "1")     # the chunked sweep pins tilings / chunk lengths through the tuning hooks
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ddsp_pytorch_amd as ddsp  # noqa: E402
from ddsp_pytorch_amd import synthetic as syn  # noqa: E402
from oracle import oracle  # noqa: E402
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import osc_grad_reference as R  # noqa: E402
import noise_grad_reference as R_noise  # noqa: E402
import noise_fwd_reference as R_nfwd  # noqa: E402
import gru_reference as R_gru  # noqa: E402
import encoder_reference as R_enc  # noqa: E402
import griffinlim_reference as R_gl  # noqa: E402
import mss_reference as R_mss  # noqa: E402


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def sweep(cases: int, seed: int, verbose: bool = True):
    """-> (failed, worst audio error, worst noise error)"""
    rng = np.random.default_rng(seed)
    worst_osc = worst_noise = 0.0
    bad = 0
    for i in range(cases):
        hop = int(rng.choice([1, 2, 3, 7, 16, 48, 64, 100, 128, 160, 256, 441, 480, 512, 1024]))
        sr = int(rng.choice([8000, 16000, 22050, 44100, 48000]))
        H = int(rng.integers(1, 241))
        B = int(rng.integers(1, 5))
        T = int(rng.integers(1, max(2, min(60, 40000 // (hop * max(1, H // 8) + 1) + 2))))
        kind = "musical" if rng.random() < 0.5 else "all_live"
        shape = syn.SynthShape("fz", B, sr, hop, T, H, 2)
        ctl = syn.make_controls(shape, int(rng.integers(1 << 30)), kind)
        if rng.random() < 0.2:
            ctl["f0"][0, T // 2:, 0] = 0.0                         # a silent stretch
        if rng.random() < 0.2:
            ctl["c"][:, :, rng.integers(0, H)] = 0.0                # an exactly-zero harmonic
        if rng.random() < 0.3:                                      # loudness spread over seven decades from frame to frame
            ctl["a"] = ctl["a"] * (10.0 ** rng.uniform(-4, 3, size=ctl["a"].shape)).astype(np.float32)
        ref, dbg = oracle.osc_forward(ctl["f0"], ctl["c"], ctl["a"], hop, sr, debug=True)
        dev = {k: torch.from_numpy(v).cuda() for k, v in ctl.items()}
        small = B * T * hop * H <= 4_000_000
        y, _, phi = ddsp.osc_forward(dev["f0"], dev["c"], dev["a"], hop, sr, debug_phases=small)
        y2, _, _ = ddsp.osc_forward(dev["f0"], dev["c"], dev["a"], hop, sr)      # production (FAST) kernels
        ok_phi = True if not small else np.array_equal(bits(phi.cpu().numpy()), bits(dbg["phi"]))
        fin = np.isfinite(ref)
        # per sample, relative to the loudness around it (the audio is the interpolated loudness x a sum of unit-range terms)
        a2 = ctl["a"][:, :, 0]
        around = np.repeat(np.maximum.reduce([a2, np.roll(a2, 1, axis=1), np.roll(a2, -1, axis=1)]), hop, axis=1)
        e_osc = float(np.max((np.abs(y2.cpu().numpy() - ref) / around)[fin])) if fin.any() else 0.0
        same_nan = np.array_equal(np.isnan(ref), np.isnan(y2.cpu().numpy()))
        # noise
        nhop = int(rng.choice([8, 16, 40, 64, 128, 256, 256, 512, 512, 512]))
        F = int(rng.integers(2, min(300, 2 * nhop) + 1))
        Tn = T
        if rng.random() < 0.3:                                      # the benchmarked kernel forms: wavefront-private / in-LDS FFT
            nhop, F = [(128, 65), (128, 65), (512, 257), (512, 195)][int(rng.integers(4))]
            Tn = int(rng.integers(1, 70))                           # whole groups of 16 frames + a ragged remainder
            if F in (195,) or (nhop == 512 and rng.random() < 0.3):     # >= 4 096 frames: the whole-batch matrix-product form (193..224 bands)
                if rng.random() < 0.15:
                    F = int(rng.integers(193, 225)) if rng.random() < 0.5 else 195
                    Tn = int(rng.integers(4096 // B + 1, 4096 // B + 12))
        Hn = syn.controller_range(rng.standard_normal((B, Tn, F), dtype=np.float32))
        level = np.ones((B, Tn, 1), dtype=np.float32)
        if rng.random() < 0.3:                                      # frames of very different level, exactly-zero bands
            level = (10.0 ** rng.uniform(-4, 3, size=(B, Tn, 1))).astype(np.float32)
            Hn *= level
            Hn[:, :, rng.integers(0, F)] = 0.0
        if rng.random() < 0.3:                                      # the in-kernel draw, regenerated by the oracle
            sd, off = int(rng.integers(1 << 40)), int(rng.integers(1 << 40))
            nref = oracle.noise_forward(Hn, None, nhop, seed=sd, offset=off)
            ny = ddsp.noise_forward(torch.from_numpy(Hn).cuda(), nhop, seed=sd, offset=off)
        else:
            u = rng.random((B, Tn, nhop), dtype=np.float32)
            nref = oracle.noise_forward(Hn, u, nhop)
            ny = ddsp.noise_forward(torch.from_numpy(Hn).cuda(), nhop, uniform=torch.from_numpy(u).cuda())
        # per frame, relative to the larger of the frame's level and its peak (all ones / the clip's peak without the level sweep)
        nerr = np.abs(ny.cpu().numpy() - nref).reshape(B, Tn, nhop).max(axis=2)
        npeak = np.abs(nref).reshape(B, Tn, nhop).max(axis=2)
        scale = np.maximum(level[:, :, 0], npeak)
        e_noise = float(np.max(nerr / scale))
        okay = ok_phi and same_nan and e_osc <= 1e-5 and e_noise <= 2e-6
        bad += not okay
        worst_osc, worst_noise = max(worst_osc, e_osc), max(worst_noise, e_noise)
        if verbose or not okay:
            print(f"{'ok ' if okay else 'BAD'} osc B{B} T{T} H{H} hop{hop} sr{sr} {kind}: phases {'bit-exact' if ok_phi else 'DIFFER'}"
                  f"{'' if small else ' (not dumped)'}, |dy| {e_osc:.1e} | noise T{Tn} hop{nhop} F{F}: {e_noise:.1e}", flush=True)
    return bad, worst_osc, worst_noise


def sweep_chunked(cases: int, seed: int, verbose: bool = True):
    """Random shapes of the CHUNKED oscillator form (csrc/ddsp_osc_chunk.hip) against the C oracle: power-of-two hops 64..2048,
    4 / 8 / 16 lanes per row (harmonics per lane pinned through the tuning hook so that small problems take it too), random
    chunk lengths (every offset of a chunk boundary inside a segment, one to many rounds of wavefronts), ragged row blocks,
    silent stretches, exactly-zero harmonics, loudness over seven decades, negative / huge / NaN f0 (the repair launch).
    -> (failed, worst audio error)"""
    L = ddsp._lib.lib()
    assert L.ddsp_test_hooks_enabled() == 1
    rng = np.random.default_rng(seed)
    worst = 0.0
    bad = 0
    Ks = [4, 8, 12, 13, 15, 16, 20, 23, 25]
    try:
        for i in range(cases):
            hop = int(rng.choice([64, 128, 128, 256, 512, 512, 1024, 2048]))
            sr = int(rng.choice([8000, 16000, 22050, 44100, 48000]))
            while True:                                          # (K, lanes) with 4, 8 or 16 lanes per row
                K = int(rng.choice(Ks))
                G = int(rng.choice([4, 8, 16]))
                H = int(rng.integers(K * (G // 2) + 1, K * G + 1))
                if H <= 400:
                    break
            B = int(rng.integers(1, 40))
            T = int(rng.integers(1, max(2, min(80, 3_000_000 // (hop * H * B) + 2))))
            kind = "musical" if rng.random() < 0.6 else "all_live"
            shape = syn.SynthShape("fz", B, sr, hop, T, H, 2)
            ctl = syn.make_controls(shape, int(rng.integers(1 << 30)), kind)
            if rng.random() < 0.2:
                ctl["f0"][0, T // 2:, 0] = 0.0
            if rng.random() < 0.2:
                ctl["c"][:, :, rng.integers(0, H)] = 0.0
            if rng.random() < 0.3:
                ctl["a"] = ctl["a"] * (10.0 ** rng.uniform(-4, 3, size=ctl["a"].shape)).astype(np.float32)
            odd = rng.random()
            if odd < 0.08:
                ctl["f0"][B - 1, rng.integers(0, T), 0] = -150.0   # phases run backwards: declined, repaired exactly
            elif odd < 0.16:
                ctl["f0"][B - 1, :, 0] *= 300.0                    # masked harmonics still accumulate phase: beyond 1e7 rad on long clips
            elif odd < 0.2:
                ctl["f0"][B - 1, rng.integers(0, T), 0] = np.nan
            n = T * hop
            lens = [v for v in range(hop, n + 32, 32)]
            os.environ["DDSP_OSC_CHUNK_LEN"] = str(int(rng.choice(lens))) if rng.random() < 0.7 else "0"
            assert L.ddsp_osc_set_tiling(K) == 0 and L.ddsp_osc_set_path(2) == 0
            plan = ddsp._lib.osc_plan(B, T, H, hop, sr)
            if not plan["chunked"] or plan["lanes_per_row"] != G:
                continue                                           # (H / K fell on another lane count: not this sweep's business)
            ref = oracle.osc_forward(ctl["f0"], ctl["c"], ctl["a"], hop, sr)
            dev = {k: torch.from_numpy(v).cuda() for k, v in ctl.items()}
            y = ddsp.osc_forward(dev["f0"], dev["c"], dev["a"], hop, sr)[0].cpu().numpy()
            fin = np.isfinite(ref)
            a2 = np.abs(ctl["a"][:, :, 0])
            around = np.repeat(np.maximum.reduce([a2, np.roll(a2, 1, axis=1), np.roll(a2, -1, axis=1)]), hop, axis=1)
            e = float(np.max((np.abs(y - ref) / np.maximum(around, 1e-30))[fin])) if fin.any() else 0.0
            same = np.array_equal(np.isfinite(y), fin)
            okay = same and e <= 1e-5
            bad += not okay
            worst = max(worst, e)
            if verbose or not okay:
                print(f"{'ok ' if okay else 'BAD'} chunked B{B} T{T} H{H} hop{hop} sr{sr} K{K} G{G} chunk {plan['chunk_samples']} {kind}"
                      f"{' odd-f0' if odd < 0.2 else ''}: |dy| {e:.1e}{'' if same else ' NON-FINITE PATTERN DIFFERS'}", flush=True)
    finally:
        os.environ.pop("DDSP_OSC_CHUNK_LEN", None)
        L.ddsp_osc_set_tiling(0)
        L.ddsp_osc_set_path(0)
    return bad, worst


# ---- the oscillator's backward (csrc/ddsp_osc_bwd.hip) against the fp64 reference -------------------------------------------
# Elementwise |grad - fp64| <= OSC_BWD_TOL x the frame's local yardstick (Yc for grad_c, Ya for grad_a: osc_grad_reference.py).
# Measured on an MI355X: worst 4.3e-7 (Nyquist crossings), every other family of tests/test_gpu_osc_backward.py and this sweep
# <= 2e-7; fp32 torch autograd of the restatement reaches ~2.5e-7 on the CPU.  2e-6 stays under 8x the worst measured ratio.
OSC_BWD_TOL = 2e-6
OSC_KS = (4, 8, 12, 13, 15, 16, 20, 23, 25)


def osc_bwd_variant(B, T, H, hop, sr):
    """(K, G, pow2, use_lds) of the backward launch for this shape under the current tiling hook: K and G from osc_plan, pow2 and
    use_lds by the formulas of setup_params (csrc/ddsp_osc.hip) and launch_bwd (csrc/ddsp_osc_bwd.hip)."""
    plan = ddsp._lib.osc_plan(B, T, H, hop, sr)
    K, G = plan["harmonics_per_lane"], plan["lanes_per_row"]
    pow2 = (hop & (hop - 1)) == 0 and hop >= 2 and T * hop <= (1 << 23)
    use_lds = 4 * (256 // G) * hop <= 64 * 1024
    return K, G, pow2, use_lds


def osc_exact_walk_expected(f0, H, hop, sr):
    """Whether the inputs send some wavefront of the backward down the exact-modulo walk, from how they were built: a negative
    f0, a harmonic with >= 1024 rad/sample (masked ones included: their phase still accumulates), or a harmonic whose
    accumulated phase passes the fast modulo's limit (1e7 rad) within the clip."""
    f = np.asarray(f0, np.float64)[..., 0]
    if (f < 0).any():
        return True
    fin = np.where(np.isfinite(f), f, 0.0)
    w_top = 2 * np.pi * H * fin / sr                              # rad/sample of the top harmonic, per frame
    return bool(w_top.max() >= 1024.0 or (hop * w_top.sum(axis=1)).max() >= 1e7)


def compare_osc_backward(ctl, gy, hop, sr, y, gc, ga, rows=None):
    """Device forward y [B,N] and gradients gc [B,T,H], ga [B,T,1] (NumPy) against the oracle and the fp64 reference on `rows`
    (default: all).  -> dict of the measured ratios and the checks the backward tests assert."""
    f0, c, a = ctl["f0"], ctl["c"], ctl["a"]
    B, T, H = c.shape
    rows = list(range(B)) if rows is None else list(rows)
    y64, gc64, ga64, Yc, Ya, yo = R.osc_grad_fp64(f0[rows], c[rows], a[rows], gy[rows], hop, sr, with_oracle_y=True)
    r = {"rc": R.ratio(gc[rows], gc64, Yc), "ra": R.ratio(ga[rows], ga64, Ya)}
    r["nonfinite_same"] = bool(np.array_equal(np.isfinite(gc[rows]), np.isfinite(gc64)) and
                               np.array_equal(np.isfinite(ga[rows]), np.isfinite(ga64)))
    mask = R.harmonic_mask(f0.reshape(-1, 1), H, sr).numpy().reshape(B, T, H)
    r["masked_zero"] = bool((gc[mask] == 0.0).all())
    quiet = [b for b in range(B) if not gy[b].any() and all(np.isfinite(ctl[k][b]).all() for k in ("f0", "c", "a"))]
    r["quiet_rows"] = len(quiet)
    r["quiet_zero"] = bool((gc[quiet] == 0.0).all() and (ga[quiet] == 0.0).all())
    fin = np.isfinite(yo)
    around = np.maximum(R.loudness_around(a[rows], hop), 1e-30)
    r["y_err"] = float(np.max((np.abs(y[rows] - yo) / around)[fin])) if fin.any() else 0.0
    r["y_nonfinite_same"] = bool(np.array_equal(np.isfinite(y[rows]), fin))
    return r


def osc_backward_case(ctl, gy, hop, sr, K=None, rows=None):
    """Raw launchers: ddsp_osc_forward_ex (frame-form scratch kept) + ddsp_osc_backward twice, the tiling pinned to K (if given)
    across the forward AND both backward calls (the backward re-runs pick_tiling to read the scratch's layout).
    -> compare_osc_backward's dict + K, G, pow2, use_lds, exact and whether the repeat was bit-identical."""
    L = ddsp._lib.lib()
    B, T, H = ctl["c"].shape
    d = {k: torch.from_numpy(np.ascontiguousarray(ctl[k])).cuda() for k in ("f0", "c", "a")}
    g = torch.from_numpy(np.ascontiguousarray(gy)).cuda()
    try:
        if K:
            ddsp._lib.check(L.ddsp_osc_set_tiling(K), "ddsp_osc_set_tiling")
        Kp, G, pow2, use_lds = osc_bwd_variant(B, T, H, hop, sr)
        y, _, _, scratch = ddsp.osc_forward(d["f0"], d["c"], d["a"], hop, sr, return_scratch=True)
        gc, ga = ddsp.osc_backward(g, d["f0"], d["c"], d["a"], scratch, hop, sr)
        gc2, ga2 = ddsp.osc_backward(g, d["f0"], d["c"], d["a"], scratch, hop, sr)
        torch.cuda.synchronize()
    finally:
        if K:
            L.ddsp_osc_set_tiling(0)
    gc, ga, gc2, ga2 = (x.cpu().numpy() for x in (gc, ga, gc2, ga2))
    r = compare_osc_backward(ctl, gy, hop, sr, y.cpu().numpy(), gc, ga, rows)
    r.update(K=Kp, G=G, pow2=pow2, use_lds=use_lds, exact=osc_exact_walk_expected(ctl["f0"], H, hop, sr),
             repeat_same=bool(np.array_equal(bits(gc), bits(gc2)) and np.array_equal(bits(ga), bits(ga2))))
    return r


def osc_backward_ok(r, tol=OSC_BWD_TOL):
    """The assertions every backward case makes, as one bool (the tests assert the fields one by one)."""
    return (r["rc"] <= tol and r["ra"] <= tol and r["nonfinite_same"] and r["masked_zero"] and r["quiet_zero"] and
            r["repeat_same"] and r["y_err"] <= 1e-5 and r["y_nonfinite_same"])


def sweep_osc_backward(cases: int, seed: int, verbose: bool = True):
    """Random shapes of the oscillator backward against the fp64 reference: the tiling pinned in half the cases (G of 1, 4, 8 or 16
    lanes), non-power-of-two and power-of-two hops (grad_y through LDS or global memory), silent stretches, exactly-zero harmonics,
    loudness over seven decades, a row whose upstream gradient is zero, glissandi across Nyquist, and the odd f0 of sweep_chunked
    (negative, x300, NaN).  B*N*H <= 4 M per case.  -> (failed, {family: worst max(err_c / Yc, err_a / Ya)})"""
    rng = np.random.default_rng(seed)
    worst = {}
    bad = 0
    for i in range(cases):
        hop = int(rng.choice([1, 3, 7, 48, 100, 160, 441, 480, 1600] + [2, 64, 128, 256, 512, 1024, 2048]))
        sr = int(rng.choice([8000, 16000, 22050, 44100, 48000]))
        K = None
        if rng.random() < 0.5:
            K = int(rng.choice(OSC_KS))
            G = int(rng.choice([1, 4, 8, 16]))
            H = int(rng.integers(K * G // 2 + 1, K * G + 1)) if G > 1 else int(rng.integers(1, K + 1))
        else:
            H = int(rng.integers(1, 241))
        B = int(rng.integers(1, 5))
        T = int(rng.integers(1, max(2, min(300, 4_000_000 // (B * hop * H) + 1))))
        kind = "musical" if rng.random() < 0.5 else "all_live"
        ctl = syn.make_controls(syn.SynthShape("fz", B, sr, hop, T, H, 2), int(rng.integers(1 << 30)), kind)
        gy = rng.standard_normal((B, T * hop)).astype(np.float32)
        if rng.random() < 0.2:
            ctl["f0"][0, T // 2:, 0] = 0.0
        if rng.random() < 0.2:
            ctl["c"][:, :, rng.integers(0, H)] = 0.0
        if rng.random() < 0.3:
            ctl["a"] = ctl["a"] * (10.0 ** rng.uniform(-4, 3, size=ctl["a"].shape)).astype(np.float32)
        if rng.random() < 0.2:                                      # a glissando through Nyquist: the live-harmonic count changes
            ctl["f0"][0, :, 0] = np.geomspace(0.5 * sr / (2 * H), 0.9 * sr / 2, T).astype(np.float32)
        if B > 1 and rng.random() < 0.3:
            gy[int(rng.integers(0, B))] = 0.0                        # a row with no upstream gradient: its gradient is exactly 0
        odd = rng.random()
        if odd < 0.08:
            ctl["f0"][B - 1, rng.integers(0, T), 0] = -150.0
        elif odd < 0.16:
            ctl["f0"][B - 1, :, 0] *= 300.0
        elif odd < 0.2:
            ctl["f0"][B - 1, rng.integers(0, T), 0] = np.nan
        r = osc_backward_case(ctl, gy, hop, sr, K=K)
        okay = osc_backward_ok(r) and (K is None or r["K"] == K)
        bad += not okay
        e = max(r["rc"], r["ra"])
        for fam in (f"K{r['K']}", "pow2" if r["pow2"] else "non-pow2", "grad_y in LDS" if r["use_lds"] else "grad_y global",
                    "exact" if r["exact"] else "fast", "tiling pinned" if K else "automatic tiling"):
            worst[fam] = max(worst.get(fam, 0.0), e)
        if verbose or not okay:
            print(f"{'ok ' if okay else 'BAD'} backward B{B} T{T} H{H} hop{hop} sr{sr} K{r['K']} G{r['G']} {kind}"
                  f"{' odd-f0' if odd < 0.2 else ''}: c {r['rc']:.1e} a {r['ra']:.1e} |dy| {r['y_err']:.1e} "
                  f"{'' if r['nonfinite_same'] else 'NON-FINITE PATTERN DIFFERS '}{'' if r['masked_zero'] else 'MASKED NONZERO '}"
                  f"{'' if r['quiet_zero'] else 'QUIET ROW NONZERO '}{'' if r['repeat_same'] else 'REPEAT DIFFERS'}", flush=True)
    return bad, worst


# ---- the filtered noise's backward (csrc/ddsp_noise.hip: ddsp_noise_backward_ws) against the fp64 reference ---------------------
# Elementwise |dH - fp64| <= NOISE_BWD_TOL x the frame's yardstick Y[f] (noise_grad_reference.py), and per frame max |err| <= 1e-5 x
# max |fp64| of the frame.  Exempt from the latter only: frames whose largest gradient is below NOISE_BWD_FRAME_FLOOR x Y[f] (the
# gradient cancels to a small part of its absolute sum, and any fp32 evaluation's relative error grows as eps Y / max |fp64|), and
# every frame at 2 bands, where each frame's whole gradient is one dot product of the hop's samples, dH[0] = dH[1] = sum_d x[d] g[d] / 2:
# it cancels to any degree (measured on an MI355X: 1.3e-5 of the frame's peak at 2 bands / hop 64, peak ~ 3e-3 Y, error 4.7e-8 Y).
# Measured on an MI355X (tests/test_gpu_noise_backward.py and 2 000 cases of this sweep): forms A and B <= 2e-8 of Y for frames at
# 2^-100 and above (1.6e-7 for a frame below form A's equaliser clamp, 2^-110 next to a unit row); the direct forms reach 2.4e-7 (C) and
# 4.2e-7 (D) at hops 7-8 with 35-44 bands.  There the impulse response is cropped to the hop, so only the window's edge values (~1e-3)
# are used.  The kernels form the window as 0.5 - 0.5 cospif(2 m / S) in fp32 (csrc/ddsp_noise.hip); the oracle, and with it the fp64
# reference, rounds an fp64 cosine instead.  Where the two cosines differ by an ulp near 1, the window value differs by ~1e-5 of
# itself: a definitional difference between kernel and oracle, not rounding in the kernels' sums.  One ulp on every cosine moves the
# fp64 reference by up to 1.3e-6 of Y at 35 bands / hop 7 (1e-9 at hop 512).  1e-6 is 2.4x the worst.
NOISE_BWD_TOL = 1e-6
NOISE_BWD_FRAME_REL = 1e-5
NOISE_BWD_FRAME_FLOOR = 1e-3


def noise_bwd_lpf_log(F, hop):
    """pick_bwd_lpf_log (csrc/ddsp_noise_plan.h): log2 lanes per frame of the batched backward, -1 when no tile fits in LDS."""
    S = 2 * (F - 1)
    for limit in (48 * 1024, 80 * 1024, 160 * 1024):
        for l in range(4):
            fb = 64 >> l
            if 4 * (((S + 3) & ~3) + fb * (hop + 4) + fb * (hop + 12) + (S // 2 + 1) * (fb + 4)) <= limit:
                return l
    return -1


def noise_bwd_form(B, T, F, hop, mode=0, aligned=True):
    """The kernel form ddsp_noise_backward_ws takes: 'A' (in-LDS FFT correlation), 'B' (FFT correlation + split-bf16 product),
    'C0'..'C3' (batched direct kernel, log2 lanes per frame), 'D' (one frame per workgroup) -- by the conditions of plan_noise_backward
    (csrc/ddsp_noise_plan.h); tests/test_noise_plan_host.py holds the two against each other."""
    if not mode & 3 and hop == 512 and aligned:
        if not mode & 16 and ddsp._lib.lib().ddsp_noise_workspace_bytes(B, T, F, hop) > 0:
            return "B"
        if 2 * (F - 1) == 512:
            return "A"
    lpf = noise_bwd_lpf_log(F, hop)
    if not mode & 1 and hop % 8 == 0 and lpf >= 0:
        return f"C{lpf}"
    return "D"


def misaligned(a):
    """A contiguous CUDA copy of `a` whose data starts 4 bytes into its storage (not 16-byte aligned)."""
    a = torch.as_tensor(np.ascontiguousarray(a))
    buf = torch.empty(a.numel() + 1, dtype=a.dtype, device="cuda")
    v = buf[1:].view(a.shape)
    v.copy_(a.cuda())
    assert v.is_contiguous() and v.data_ptr() % 16 != 0
    return v


def noise_backward_run(gy, F, hop, uniform=None, seed=0, offset=0, counter=None, mode=0, misalign=()):
    """Two launches of ddsp.noise_backward under ddsp_noise_set_generic(mode) -> (dH, repeat) as NumPy.  `misalign`: the names
    of the inputs ('grad_y', 'uniform') passed as views 4 bytes into their storage."""
    L = ddsp._lib.lib()

    def put(a, name):
        return misaligned(a) if name in misalign else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    g = put(gy, "grad_y")
    kw = dict(uniform=put(uniform, "uniform")) if uniform is not None else dict(seed=seed, offset=offset)
    if counter is not None:
        kw["counter"] = torch.tensor([counter], dtype=torch.int64, device="cuda")
    try:
        ddsp._lib.check(L.ddsp_noise_set_generic(mode), "ddsp_noise_set_generic")
        a = ddsp.noise_backward(g, hop, F, **kw)
        b = ddsp.noise_backward(g, hop, F, **kw)
        torch.cuda.synchronize()
    finally:
        L.ddsp_noise_set_generic(0)
    return a.cpu().numpy(), b.cpu().numpy()


def compare_noise_backward(got, ref, Y, gy, hop, paired=False):
    """Device dH [B,T,F] against the fp64 reference (ref, Y) -> dict of the measured ratios and the checks the tests assert.
    `paired`: the kernel shares transforms between frames 2p and 2p + 1 (forms A and B, ddsp_noise_fft.hip: load_rows), so the
    partner of a frame with a non-finite gradient may come out entirely non-finite; never finite and wrong."""
    B, T, F = ref.shape
    g = np.asarray(gy, np.float32).reshape(B * T, hop)
    got, ref, Y = got.reshape(B * T, F), ref.reshape(B * T, F), Y.reshape(B * T)
    bad = ~np.isfinite(g).all(axis=1)
    partner = np.zeros_like(bad)
    if paired:
        idx = np.flatnonzero(bad)
        partner[np.minimum(idx ^ 1, B * T - 1)] = True       # (an odd last frame is paired with itself)
        partner &= ~bad
    fin_got = np.isfinite(got).all(axis=1)
    lost = partner & ~np.isfinite(got).any(axis=1)            # partners that came out entirely non-finite
    judged = ~bad & ~lost
    r = {"frames": B * T, "bad_frames": int(bad.sum()), "partners_lost": int(lost.sum())}
    r["nonfinite_ok"] = bool((~np.isfinite(got[bad])).all() and fin_got[judged].all())
    per = R_noise.ratio(got[judged], ref[judged], Y[judged])
    r["ratio"] = float(per.max()) if per.size else 0.0
    err = np.abs(got[judged] - ref[judged]).max(axis=1) if F else np.zeros(0)
    peak = np.abs(ref[judged]).max(axis=1)
    keep = (peak >= NOISE_BWD_FRAME_FLOOR * Y[judged]) & (F > 2)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(err[keep] == 0.0, 0.0, err[keep] / peak[keep])
    r["frame_rel"] = float(np.nan_to_num(rel, nan=np.inf).max()) if rel.size else 0.0
    zero = ~g.any(axis=1) & ~partner
    r["zero_frames"] = int(zero.sum())
    r["zero_exact"] = bool((got[zero] == 0.0).all())
    return r


def noise_backward_case(gy, F, hop, uniform=None, seed=0, offset=0, counter=None, mode=0, misalign=(), against_d=True, same_as=None):
    """ddsp.noise_backward twice (bit-identical repeat) against noise_grad_reference.noise_grad_fp64 of the same draw (the Philox
    offset includes the counter's value).  against_d: also the same call under mode 1 (the one-frame-per-workgroup kernel), which
    must meet the same contract and -- when the default took another form -- differ from it bitwise.  same_as: also the same call
    under that mode; r['same_as'] tells whether the two results are bit-identical (mode 2 forces the direct kernels: a call that
    declined forms A and B equals it, one that took them does not).  -> dict (+ 'form')."""
    g = np.ascontiguousarray(gy, np.float32)
    B, T = g.shape[0], g.shape[1] // hop
    form = noise_bwd_form(B, T, F, hop, mode, aligned="grad_y" not in misalign and (uniform is None or "uniform" not in misalign))
    ref, Y = R_noise.noise_grad_fp64(g, F, hop, uniform=uniform, seed=seed, offset=offset + (counter or 0))
    got, again = noise_backward_run(g, F, hop, uniform, seed, offset, counter, mode, misalign)
    r = compare_noise_backward(got, ref, Y, g, hop, paired=form in ("A", "B"))
    r.update(form=form, F=F, repeat_same=bool(np.array_equal(bits(got), bits(again))))
    if same_as is not None:
        other, _ = noise_backward_run(g, F, hop, uniform, seed, offset, counter, same_as, misalign)
        r["same_as"] = bool(np.array_equal(bits(got), bits(other)))
    if against_d and form != "D":
        d, _ = noise_backward_run(g, F, hop, uniform, seed, offset, counter, 1, misalign)
        rd = compare_noise_backward(d, ref, Y, g, hop)
        r["differs_from_d"] = not np.array_equal(bits(got), bits(d))
        r["d_ok"] = rd["ratio"] <= NOISE_BWD_TOL and rd["frame_rel"] <= NOISE_BWD_FRAME_REL and rd["nonfinite_ok"] and rd["zero_exact"]
        r["d_ratio"] = rd["ratio"]
    return r


def noise_backward_ok(r, tol=NOISE_BWD_TOL):
    """The assertions every noise backward case makes, as one bool (the tests assert the fields one by one)."""
    return (r["ratio"] <= tol and r["frame_rel"] <= NOISE_BWD_FRAME_REL and r["nonfinite_ok"] and r["zero_exact"] and r["repeat_same"]
            and r.get("d_ok", True) and r.get("differs_from_d", True))


def frame_levels(rng, B, T, decades=True):
    """Per-frame levels [B,T,1] of the upstream gradient: 10^U(-4,3) (seven decades), or ones."""
    if not decades:
        return np.ones((B, T, 1), np.float32)
    return (10.0 ** rng.uniform(-4, 3, size=(B, T, 1))).astype(np.float32)


def sweep_noise_backward(cases: int, seed: int, verbose: bool = True):
    """Random shapes of the noise backward against the fp64 reference: odd hops, multiples of 8, 256, 512 (every form: in-LDS FFT at
    257 bands, the split-bf16 product in the 193..224-band range at >= 512 frames, batched direct at every lane count, one frame per
    workgroup), the injected draw or the in-kernel one at 64-bit offsets (a device counter in some), frame levels over seven decades,
    zero frames, forced modes 0 / 1 / 2 / 16.  B*T*hop <= 1.5 M per case.  -> (failed, {form: worst error / yardstick})"""
    rng = np.random.default_rng(seed)
    worst = {}
    bad = 0
    for i in range(cases):
        kind = rng.random()
        if kind < 0.15:                                              # the matrix-product form's band range, >= 512 frames
            hop, F = 512, int(rng.integers(193, 225))
            n = int(rng.integers(512, 700)) if rng.random() < 0.8 else int(rng.integers(400, 512))
        elif kind < 0.3:
            hop, F = 512, 257 if rng.random() < 0.6 else int(rng.integers(2, 400))
            n = int(rng.integers(1, 120))
        else:
            hop = int(rng.choice([1, 3, 5, 7, 12, 100, 441, 8, 16, 40, 64, 128, 160, 256, 480, 1024]))
            F = int(rng.integers(2, min(1100, 2 * hop + 40) + 1))
            n = int(rng.integers(1, max(2, min(200, 1_500_000 // hop))))
        B = int(rng.choice([d for d in (1, 2, 3, 4) if n % d == 0])) if n > 3 else 1
        T = n // B
        gy = rng.standard_normal((B, T, hop)).astype(np.float32) * frame_levels(rng, B, T, rng.random() < 0.5)
        if n > 1 and rng.random() < 0.3:
            gy[rng.integers(0, B), rng.integers(0, T)] = 0.0          # a frame with no upstream gradient: exact zeros
        gy = gy.reshape(B, T * hop)
        mode = int(rng.choice([0, 0, 0, 1, 2, 16]))
        kw = {}
        if rng.random() < 0.5:
            kw["uniform"] = rng.random((B, T, hop), dtype=np.float32)
        else:
            kw["seed"], kw["offset"] = int(rng.integers(1 << 62)), int(rng.integers(1 << 62))
            if rng.random() < 0.3:
                kw["counter"] = int(rng.integers(1 << 40))
        r = noise_backward_case(gy, F, hop, mode=mode, against_d=False, **kw)
        okay = noise_backward_ok(r)
        bad += not okay
        worst[r["form"]] = max(worst.get(r["form"], 0.0), r["ratio"])
        if verbose or not okay:
            print(f"{'ok ' if okay else 'BAD'} noise backward B{B} T{T} F{F} hop{hop} mode {mode} form {r['form']} "
                  f"{'injected' if 'uniform' in kw else 'philox'}: {r['ratio']:.1e} of Y, frame {r['frame_rel']:.1e}"
                  f"{'' if r['nonfinite_ok'] else ' NON-FINITE'}{'' if r['zero_exact'] else ' ZERO FRAME NONZERO'}"
                  f"{'' if r['repeat_same'] else ' REPEAT DIFFERS'}", flush=True)
    return bad, worst


# ---- the filtered noise's forward (csrc/ddsp_noise.hip: ddsp_noise_forward_ws) against the fp64 reference -----------------------
# Per sample |y - fp64| <= TOL_SAMPLE x Y[n] (the direct forms: Batched, Frame, Wave), per frame max |err| <= TOL_FRAME x Yframe
# (every form) and max |err| <= FRAME_REL x the frame's own fp64 peak (exempt: frames with peak < FRAME_FLOOR x Yframe).  The yardsticks
# and the tolerances are tests/noise_fwd_reference.py's, derived on the host in tests/test_noise_fwd_reference_host.py.
def noise_fwd_lpf_log(F, hop, mode=0):
    """pick_lpf_log (csrc/ddsp_noise_plan.h): log2 lanes per frame of the batched forward kernel, -1 when no tile fits in LDS; a
    mode of (l + 1) << 8 forces l."""
    if mode >> 8:
        return (mode >> 8) - 1
    S = 2 * (F - 1)
    for limit in (40 * 1024, 80 * 1024, 160 * 1024):
        for l in range(4):
            fb = 64 >> l
            if 4 * (((S + 3) & ~3) + fb * (hop + 4) + max((fb + 4) * F, fb * (hop + 12))) <= limit:
                return l
    return -1


def noise_ir_product_shape(F, hop):
    """ir_product_shape (csrc/ddsp_noise_plan.h): the band range the whole-batch matrix product is built for."""
    S, NQ = 2 * (F - 1), (F - 1) // 2 + 1
    return hop == 512 and S < hop and 96 < NQ <= 112


def noise_fwd_form(B, T, F, hop, mode=0, y_aligned=True, hm_aligned=True, u_given=False, u_aligned=True, workspace=True):
    """The kernel form ddsp_noise_forward_ws takes: 'FFT' (in-LDS FFT form, cosine sums or the packed inverse FFT), 'FFT+IR' (the
    impulse responses from the split-bf16 matrix product first), 'WAVE' (wavefront-private form, whole groups of 16 frames),
    'WAVE+Cl' (... and the remainder in the batched kernel), 'C0'..'C3' (batched direct kernel, log2 lanes per frame), 'D' (one frame
    per workgroup) -- by the conditions of plan_noise_forward (csrc/ddsp_noise_plan.h); tests/test_noise_plan_host.py holds the two
    against each other.  `workspace`: a whole 16-byte-aligned workspace of ddsp_noise_workspace_bytes is passed (noise_forward does)."""
    S, frames = 2 * (F - 1), B * T
    u_ok = not u_given or u_aligned

    def direct():
        lpf = noise_fwd_lpf_log(F, hop, mode)
        return f"C{lpf}" if not mode & 1 and hop % 8 == 0 and lpf >= 0 and y_aligned else "D"
    if not mode & 3 and 4 <= S <= hop and y_aligned and u_ok and (hop == 512 or (hop == 256 and mode & 4)):
        product = not mode & 16 and noise_ir_product_shape(F, hop) and frames >= 4096 and workspace
        return "FFT+IR" if product else "FFT"
    if not mode & 9 and hop == 128 and F == 65 and y_aligned and hm_aligned and u_ok and frames >= 16:
        return "WAVE" if frames % 16 == 0 else "WAVE+" + direct()
    return direct()


def noise_forward_run(H, hop, uniform=None, seed=0, offset=0, counter=None, mode=0, misalign=(), base=None):
    """Two launches of ddsp.noise_forward under ddsp_noise_set_generic(mode), each into an output pre-filled with NaN (a path that
    writes nothing cannot pass) or, accumulating, with `base` -> (y, repeat) as NumPy.  `misalign`: the names of the arguments ('y',
    'uniform', 'Hmag') passed as views 4 bytes into their storage."""
    L = ddsp._lib.lib()
    B, T, F = H.shape

    def put(a, name):
        return misaligned(a) if name in misalign else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    Hd = put(H, "Hmag")
    kw = dict(uniform=put(uniform, "uniform")) if uniform is not None else dict(seed=seed, offset=offset)
    if counter is not None:
        kw["counter"] = torch.tensor([counter], dtype=torch.int64, device="cuda")
    fill = np.full((B, T * hop), np.nan, np.float32) if base is None else np.ascontiguousarray(base, np.float32).reshape(B, T * hop)
    outs = [put(fill, "y"), put(fill, "y")]
    try:
        ddsp._lib.check(L.ddsp_noise_set_generic(mode), "ddsp_noise_set_generic")
        for out in outs:
            ddsp.noise_forward(Hd, hop, out=out, accumulate=base is not None, **kw)
        torch.cuda.synchronize()
    finally:
        L.ddsp_noise_set_generic(0)
    return tuple(o.cpu().numpy().reshape(B, T, hop) for o in outs)


def compare_noise_forward(got, y, Y, H, paired=False, base=None):
    """Device audio [B,T,hop] against the fp64 reference (y, Y) -> dict of the measured figures and the checks the tests assert,
    with the per-frame arrays under 'per_frame' (sample, frame, rel: [B*T], NaN where not judged).
    `paired`: the kernel transforms frames 2p and 2p + 1 as one complex sequence (the Fft forms, ddsp_noise_fft.hip), so the partner
    of a frame with a non-finite H may come out entirely non-finite; never finite and wrong.  `base`: the output's earlier contents
    (accumulate): the reference is base + y and every bound gains the sum's own rounding, 2^-24 (|base| + |y|) per sample."""
    B, T, F = H.shape
    n, hop = B * T, y.shape[-1]
    got = np.asarray(got, np.float64).reshape(n, hop)
    y, Y, Hf = y.reshape(n, hop), Y.reshape(n, hop), H.reshape(n, F)
    bad = ~np.isfinite(Hf).all(axis=1)
    partner = np.zeros_like(bad)
    if paired:
        idx = np.flatnonzero(bad)
        partner[np.minimum(idx ^ 1, n - 1)] = True              # (an odd last frame is paired with itself)
        partner &= ~bad
    lost = partner & ~np.isfinite(got).any(axis=1)              # partners that came out entirely non-finite
    judged = ~bad & ~lost
    r = {"frames": n, "bad_frames": int(bad.sum()), "partners_lost": int(lost.sum())}
    r["nonfinite_ok"] = bool((~np.isfinite(got[bad])).all() and np.isfinite(got[judged]).all())
    want, extra = y, 0.0
    if base is not None:
        b = np.asarray(base, np.float64).reshape(n, hop)
        with np.errstate(invalid="ignore"):
            want, extra = b + y, 2.0 ** -24 * (np.abs(b) + np.abs(y))
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.maximum(np.abs(got - want) - extra, 0.0)
        err[~np.isfinite(got)] = np.inf
        Yf, peak = Y.max(axis=1), np.abs(y).max(axis=1)
        sample = np.where(err == 0.0, 0.0, err / Y).max(axis=1)
        emax = err.max(axis=1)
        frame = np.where(emax == 0.0, 0.0, emax / Yf)
        rel = np.where(emax == 0.0, 0.0, emax / peak)
    keep = judged & ((peak >= R_nfwd.FRAME_FLOOR * Yf) | (emax == 0.0))
    for a in (sample, frame):
        a[~judged] = np.nan
        a[judged & np.isnan(a)] = np.inf
    rel[~keep] = np.nan
    rel[keep & np.isnan(rel)] = np.inf
    worst = lambda a: float(np.nanmax(a)) if np.isfinite(a).any() or np.isinf(a).any() else 0.0      # noqa: E731
    r.update(ratio_sample=worst(sample), ratio_frame=worst(frame), frame_rel=worst(rel),
             exempt_frames=int((judged & ~keep).sum()))
    zero = ~Hf.any(axis=1) & ~partner
    r["zero_frames"] = int(zero.sum())
    r["zero_exact"] = bool((got[zero] == (0.0 if base is None else np.asarray(base, np.float64).reshape(n, hop)[zero])).all())
    r["per_frame"] = dict(sample=sample, frame=frame, rel=rel)
    return r


def noise_forward_meets(r, direct):
    """The numeric contract as one bool: every form per frame, the direct forms per sample as well."""
    ok = r["ratio_frame"] <= R_nfwd.TOL_FRAME and (not direct or r["ratio_sample"] <= R_nfwd.TOL_SAMPLE)
    return bool(ok and r["frame_rel"] <= R_nfwd.FRAME_REL and r["nonfinite_ok"] and r["zero_exact"])


def noise_forward_case(H, hop, uniform=None, seed=0, offset=0, counter=None, mode=0, misalign=(), accumulate=None, against_d=True,
                       same_as=None):
    """ddsp.noise_forward twice (bit-identical repeat) against noise_fwd_reference.noise_fwd_fp64 of the same draw (the Philox offset
    includes the counter's value).  accumulate: the output's earlier contents [B, T*hop].  against_d: also the same call under mode 1
    (the one-frame-per-workgroup kernel), which must meet the same contract and -- when the default took another form -- differ from
    it bitwise.  same_as: also the same call under that mode; r['same_as'] tells whether the two results are bit-identical.
    -> dict (+ 'form', 'direct', and 'parts': {family: (ratio_sample, ratio_frame, frame_rel)} -- one family per kernel that ran:
    the remainder of a 'WAVE+Cl' call is judged as its own family)."""
    H = np.ascontiguousarray(H, np.float32)
    B, T, F = H.shape
    form = noise_fwd_form(B, T, F, hop, mode, y_aligned="y" not in misalign, hm_aligned="Hmag" not in misalign,
                          u_given=uniform is not None, u_aligned="uniform" not in misalign)
    direct = not form.startswith("FFT")
    y, Y = R_nfwd.noise_fwd_fp64(H, hop, uniform=uniform, seed=seed, offset=offset + (counter or 0))
    got, again = noise_forward_run(H, hop, uniform, seed, offset, counter, mode, misalign, accumulate)
    r = compare_noise_forward(got, y, Y, H, paired=not direct, base=accumulate)
    r.update(form=form, direct=direct, F=F, repeat_same=bool(np.array_equal(bits(got), bits(again))))
    pf = r.pop("per_frame")

    def part(sl):
        w = lambda a: float(np.nanmax(a[sl])) if (~np.isnan(a[sl])).any() else 0.0      # noqa: E731
        return (w(pf["sample"]) if direct else 0.0, w(pf["frame"]), w(pf["rel"]))
    if form.startswith("WAVE+"):
        done = (B * T) - (B * T) % 16
        r["parts"] = {"WAVE": part(slice(0, done)), form: part(slice(done, None))}
    else:
        r["parts"] = {form: part(slice(None))}
    r["ok"] = noise_forward_meets(r, direct)
    if same_as is not None:
        other, _ = noise_forward_run(H, hop, uniform, seed, offset, counter, same_as, misalign, accumulate)
        r["same_as"] = bool(np.array_equal(bits(got), bits(other)))
    if against_d and form != "D":
        d, _ = noise_forward_run(H, hop, uniform, seed, offset, counter, 1, misalign, accumulate)
        rd = compare_noise_forward(d, y, Y, H, base=accumulate)
        rd.pop("per_frame")
        r["differs_from_d"] = not np.array_equal(bits(got), bits(d))
        r["d_ok"] = noise_forward_meets(rd, True)
        r["d_ratio"] = rd["ratio_sample"]
        r["d_figures"] = {k: rd[k] for k in ("ratio_sample", "ratio_frame", "frame_rel", "nonfinite_ok", "zero_exact")}
    return r


def noise_forward_ok(r):
    """The assertions every noise forward case makes, as one bool (the tests assert the fields one by one)."""
    return bool(r["ok"] and r["repeat_same"] and r.get("d_ok", True) and r.get("differs_from_d", True))


def sweep_noise_forward(cases: int, seed: int, verbose: bool = True):
    """Random shapes of the noise forward against the fp64 reference: the backward sweep's pool of shapes (odd hops, multiples of 8,
    256, 512; the matrix-product band range below its 4 096 frames, which 1.5 M samples leave no room for), hop 128 / 65 bands at 1 .. 200 frames (the wavefront form and its
    remainder) and the FFT form at hop 256 (mode 4); H at frame levels over seven decades, a zero frame in some; the injected draw or
    the in-kernel one at 64-bit offsets (a device counter in some); modes 0 / 1 / 2 / 4 / 8 / 16 / forced lane counts.  B*T*hop <= 1.5 M
    per case.  -> (failed, {form: worst error / yardstick: Y[n] for the direct forms, Yframe for the Fft forms})"""
    rng = np.random.default_rng(seed)
    worst = {}
    bad = 0
    for i in range(cases):
        kind = rng.random()
        mode = int(rng.choice([0, 0, 0, 1, 2, 8, 16]))
        if kind < 0.04:                                              # the matrix-product form's band range just below its 4 096 frames (1.5 M samples): declined
            hop, F, n = 512, int(rng.integers(193, 225)), int(rng.integers(2900, 2930))
        elif kind < 0.2:
            hop, F = 512, int(rng.choice([257, 195, 129, 256, 3, int(rng.integers(2, 400))]))
            n = int(rng.integers(1, 60))
        elif kind < 0.4:
            hop, F, n = 128, 65, int(rng.integers(1, 201))
        elif kind < 0.5:
            hop, F, n, mode = 256, int(rng.integers(3, 130)), int(rng.integers(1, 60)), 4
        else:
            hop = int(rng.choice([1, 3, 5, 7, 12, 100, 441, 8, 16, 40, 64, 128, 160, 256, 480, 1024]))
            F = int(rng.integers(2, min(1100, 2 * hop + 40) + 1))
            n = int(rng.integers(1, max(2, min(200, 1_500_000 // hop))))
            if rng.random() < 0.3 and hop % 8 == 0:
                l = int(rng.integers(0, 4))
                fb = 64 >> l
                if 4 * (((2 * F + 1) & ~3) + fb * (hop + 4) + max((fb + 4) * F, fb * (hop + 12))) <= 160 * 1024:
                    mode = (l + 1) << 8                              # a forced lane count whose tile fits in LDS
        B = int(rng.choice([d for d in (1, 2, 3, 4) if n % d == 0])) if n > 3 else 1
        T = n // B
        H = syn.controller_range(rng.standard_normal((B, T, F), dtype=np.float32)) * frame_levels(rng, B, T, rng.random() < 0.7)
        if n > 1 and rng.random() < 0.3:
            H[rng.integers(0, B), rng.integers(0, T)] = 0.0           # a silent frame: exact zeros
        kw = {}
        if rng.random() < 0.5:
            kw["uniform"] = rng.random((B, T, hop), dtype=np.float32)
        else:
            kw["seed"], kw["offset"] = int(rng.integers(1 << 62)), int(rng.integers(1 << 62))
            if rng.random() < 0.3:
                kw["counter"] = int(rng.integers(1 << 40))
        r = noise_forward_case(H, hop, mode=mode, against_d=False, **kw)
        okay = noise_forward_ok(r)
        bad += not okay
        for fam, (rs, rf, _) in r["parts"].items():
            worst[fam] = max(worst.get(fam, 0.0), rs if r["direct"] else rf)
        if verbose or not okay:
            print(f"{'ok ' if okay else 'BAD'} noise forward B{B} T{T} F{F} hop{hop} mode {mode} form {r['form']} "
                  f"{'injected' if 'uniform' in kw else 'philox'}: {r['ratio_sample']:.1e} of Y[n], {r['ratio_frame']:.1e} of Yframe, "
                  f"{r['frame_rel']:.1e} of the peak{'' if r['nonfinite_ok'] else ' NON-FINITE'}"
                  f"{'' if r['zero_exact'] else ' ZERO FRAME NONZERO'}{'' if r['repeat_same'] else ' REPEAT DIFFERS'}", flush=True)
    return bad, worst


# ---- the GRU recurrence (csrc/ddsp_gru.hip) step by step against the fp64 reference of tests/gru_reference.py -------------------
def gru_case(B, T, Hd, lowp, seed, h0=True, bias=True, dhT=True, io16=None, spread=False, keep=False):
    """One forward (saving and not saving) and one backward of the raw launchers on the inputs of gru_reference.make_inputs, against
    the teacher-forced fp64 reference with the rounding gru_reference.plan predicts for every batch row.  `io16` (default: with
    every bf16 backward): the same backward with 16-bit d_gi / d_gh.  `spread`: under ddsp_gru_set_mode(1).
    -> dict: plan_fwd / plan_bwd (lists of Slice), fwd / bwd ({tensor: Measure}), bad (messages: empty when every check of the
    criterion holds -- bounds, non-vacuity, status words, hT == y[:, -1] and save=False == save=True bitwise, the io16 checks);
    keep: + 'out', the device tensors (y, hT, gates, hn, d_gi, d_gh, dh0)."""
    from ddsp_pytorch_amd import gru as gru_mod
    L = ddsp._lib.lib()
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    x = R_gru.make_inputs(B, T, Hd, seed, h0, bias, dhT)
    d = {k: (None if v is None else v.cuda()) for k, v in x.items()}
    r = {"plan_fwd": R_gru.plan(B, Hd, cus, lowp, False, spread, T), "plan_bwd": R_gru.plan(B, Hd, cus, lowp, True, spread, T)}
    bwd_mfma = all(s.mfma for s in r["plan_bwd"])
    io16 = lowp if io16 is None else (io16 and lowp)
    used = []
    try:
        if spread:
            ddsp._lib.check(L.ddsp_gru_set_mode(1), "ddsp_gru_set_mode")
        y, hT, gates, hn = gru_mod.gru_forward(d["gi"], d["w"], d["b"], d["h0"], save=True, scratch_out=used, lowp=lowp)
        y2, hT2, g2, hn2 = gru_mod.gru_forward(d["gi"], d["w"], d["b"], d["h0"], save=False, scratch_out=used, lowp=lowp)
        d_gi, d_gh, dh0 = gru_mod.gru_backward(d["dy"], d["dhT"], d["w"], d["h0"], y, gates, hn, scratch_out=used, lowp=lowp)
        if io16:
            h_gi, h_gh, h_dh0 = gru_mod.gru_backward(d["dy"], d["dhT"], d["w"], d["h0"], y, gates, hn, scratch_out=used, lowp=True, io16=True)
        status = [gru_mod.gru_status(s) for s in used]
    finally:
        if spread:
            L.ddsp_gru_set_mode(0)
    bad = []
    if any(status):
        bad.append(f"status words {status}")
    if g2 is not None or hn2 is not None:
        bad.append("save=False returned saved tensors")
    if not torch.equal(hT, y[:, -1]):
        bad.append("hT != y[:, -1]")
    if not (torch.equal(y, y2) and torch.equal(hT, hT2)):
        bad.append("save=False differs from save=True")
    c = lambda t: t.cpu()      # noqa: E731
    yc, gc, hnc = c(y), c(gates), c(hn)
    rows_f, rows_b = R_gru.rounded_rows(r["plan_fwd"]), R_gru.rounded_rows(r["plan_bwd"])
    r["fwd"] = R_gru.forward_measures(x, yc, c(hT), gc, hnc, rows_f)
    r["bwd"] = R_gru.backward_measures(x, yc, gc, hnc, c(d_gi), c(d_gh), c(dh0), rows_b)
    bad += ["forward " + m for m in R_gru.failures(r["fwd"], T)] + ["backward " + m for m in R_gru.failures(r["bwd"], T)]
    if io16:
        if h_gi.dtype != torch.bfloat16 or h_gh.dtype != torch.bfloat16:
            bad.append("io16 outputs are not bf16")
        if not torch.equal(h_dh0, dh0):
            bad.append("io16: dh0 differs from the fp32-output launch")
        if bwd_mfma:
            # one bf16 ulp of the reference teacher-forced from the 16-bit d_gh itself: half an ulp of the kernel's fp32 value (its
            # rounding to bf16) + that value's own fp32 error, which the criterion bounds by MARGIN x e32 of the tensor's largest entry
            args = (x["dy"], x["dhT"], x["w"], x["h0"], yc, gc, hnc, c(h_gh))
            ref = R_gru.backward_steps(*args, torch.float64, rows_b)
            ref32 = R_gru.backward_steps(*args, torch.float32, rows_b)
            for name, got, want, w32 in zip(("d_gi", "d_gh"), (h_gi, h_gh), ref, ref32):
                top = float(want.abs().max())
                tol = R_gru.bf16_ulp(want) + R_gru.MARGIN * float((w32.double() - want).abs().max())
                over = float(((c(got).double() - want).abs() - tol).max())
                r["io16_" + name] = float(((c(got).double() - want).abs() / tol).max())       # <= 1 passes
                if not over <= 0.0:
                    bad.append(f"io16 {name}: {over:.3e} (of a largest entry {top:.3e}) beyond one bf16 ulp of the reference")
            if not float((c(h_dh0).double() - ref[2]).abs().max()) <= R_gru.MARGIN * float((ref32[2].double() - ref[2]).abs().max()):
                bad.append("io16 dh0 against the reference teacher-forced from the 16-bit d_gh")
        else:   # T >= 65536: the fp32 backward ran and gru.py cast its outputs
            if not (torch.equal(h_gi, d_gi.to(torch.bfloat16)) and torch.equal(h_gh, d_gh.to(torch.bfloat16))):
                bad.append("io16 fallback: not the bf16 cast of the fp32 outputs")
    r["bad"] = bad
    r["ratio_fwd"], r["ratio_bwd"] = R_gru.worst_ratio(r["fwd"]), R_gru.worst_ratio(r["bwd"])
    r["family_fwd"] = ("bf16" if any(s.mfma for s in r["plan_fwd"]) else "fp32") + " forward"
    r["family_bwd"] = ("bf16" if bwd_mfma else "fp32") + " backward"
    if keep:
        r["out"] = (y, hT, gates, hn, d_gi, d_gh, dh0)
    return r


def gru_case_line(r):
    return (f"{r['family_fwd']} {'+'.join(s.kernel for s in r['plan_fwd'])} BL {[s.BL for s in r['plan_fwd']]} last {[s.last for s in r['plan_fwd']]}: "
            f"{r['ratio_fwd']:.2f} x e32 [{R_gru.describe(r['fwd'])}] | {r['family_bwd']} {'+'.join(s.kernel for s in r['plan_bwd'])} "
            f"BL {[s.BL for s in r['plan_bwd']]}: {r['ratio_bwd']:.2f} x e32 [{R_gru.describe(r['bwd'])}]"
            + "".join(f" | {k} {v:.2f} of (1 bf16 ulp + the fp32 bound)" for k, v in r.items() if k.startswith("io16_")))


def sweep_gru(cases: int, seed: int, verbose: bool = True, counts: dict | None = None):
    """Random shapes of the GRU recurrence against the fp64 reference: Hd in 1 .. 512 (the four KP classes equally often, so that a
    short sweep reaches every instantiation's class), B in 1 .. 300, T in 1 .. 12, random lowp / h0 / bias / dhT / io16.  (T = 1
    without h0 multiplies W_hh by zeros only -- no rounding to tell apart, the non-vacuity condition cannot hold: such a draw gets
    an h0.)  `counts` receives {kernel instantiation: launches' cases}.  -> (failed, {family: worst error / e32})"""
    rng = np.random.default_rng(seed)
    worst = {}
    counts = {} if counts is None else counts
    bad = 0
    for i in range(cases):
        lo, hi = [(1, 64), (65, 128), (129, 256), (257, 512)][int(rng.integers(4))]
        Hd = int(rng.integers(lo, hi + 1))
        B = int(rng.integers(1, 301))
        T = int(rng.integers(1, 13))
        lowp, h0, bias, dhT, io16 = (bool(rng.random() < 0.5) for _ in range(5))
        h0 = h0 or T == 1
        r = gru_case(B, T, Hd, lowp, int(rng.integers(1 << 30)), h0=h0, bias=bias, dhT=dhT, io16=io16)
        okay = not r["bad"]
        bad += not okay
        for s in r["plan_fwd"] + r["plan_bwd"]:
            counts[s.kernel] = counts.get(s.kernel, 0) + 1
        worst[r["family_fwd"]] = max(worst.get(r["family_fwd"], 0.0), r["ratio_fwd"])
        worst[r["family_bwd"]] = max(worst.get(r["family_bwd"], 0.0), r["ratio_bwd"])
        if verbose or not okay:
            print(f"{'ok ' if okay else 'BAD'} gru B{B} T{T} Hd{Hd} lowp {int(lowp)} h0 {int(h0)} bias {int(bias)} dhT {int(dhT)} io16 {int(io16)}: "
                  f"{gru_case_line(r)}{'' if okay else ' ' + '; '.join(r['bad'])}", flush=True)
    if verbose:
        print("kernel instantiations reached: " + ", ".join(f"{k} x{v}" for k, v in sorted(counts.items())), flush=True)
    return bad, worst


def sweep_training_kernels(cases: int, seed: int, verbose: bool = True):
    """Random shapes of the loss-side kernels against torch on the CPU in fp64: ddsp_mss_scale (+ the overlap-add gather) for random
    batch / length / transform size / overlap, the framing pair around a library rfft, and the column sums.  -> failed cases"""
    from ddsp_pytorch_amd import dense
    from ddsp_pytorch_amd.training import SpectralLoss
    rng = np.random.default_rng(seed)
    g = torch.Generator().manual_seed(seed)
    bad = 0
    ratios = []
    for i in range(cases):
        n_fft = int(rng.choice([64, 128, 256, 512, 1024, 2048]))
        overlap = float(rng.choice([0.75, 0.75, 0.5, 0.875, 0.0]))
        B = int(rng.integers(1, 6))
        L = int(rng.integers(n_fft // 2 + 1, n_fft // 2 + 1 + int(rng.choice([3, 200, 5000]))))
        x_true = 0.3 * torch.randn(B, L, generator=g)
        x_pred = 0.3 * torch.randn(B, L, generator=g)
        if rng.random() < 0.3:
            x_true[0, : L // 2] = 0.0
        sl = SpectralLoss(n_fft, alpha=float(rng.choice([1.0, 0.3])), overlap=overlap)
        xp = x_pred.double().requires_grad_(True)
        ref = sl.double()(xp, x_true.double())
        ref.backward()
        sl_gpu = SpectralLoss(n_fft, alpha=sl.alpha, overlap=overlap).cuda()
        xg = x_pred.cuda().requires_grad_(True)
        fused = sl_gpu.fused_scale(xg) is not None
        got = sl_gpu(xg, x_true.cuda())
        got.backward()
        e_loss = abs(got.item() - ref.item()) / abs(ref.item())
        gd = xg.grad.cpu().double() - xp.grad
        e_l2 = float(gd.norm() / xp.grad.norm())
        e_max = float(gd.abs().max() / xp.grad.abs().max())
        # the yardstick: what fp32 arithmetic does to this gradient in the torch formulation itself (the log term goes like
        # 1 / (|S|^2 + eps) per bin: one near-empty bin of the prediction and any fp32 transform is off by 1e-3 of the norm)
        x32 = x_pred.clone().requires_grad_(True)
        SpectralLoss(n_fft, alpha=sl.alpha, overlap=overlap)(x32, x_true).backward()
        d32 = x32.grad.double() - xp.grad
        y_l2, y_max = float(d32.norm() / xp.grad.norm()), float(d32.abs().max() / xp.grad.abs().max())
        # ... and the conditioning of the case itself: the L1 terms' gradient is discontinuous where a bin of the prediction ties
        # with the target's (sign(P - Q), sign(log Q - log P)); an fp32-epsilon perturbation of the INPUT, evaluated in fp64,
        # shows how much of the gradient such near-ties decide (single-frame and half-silent cases reach 1e-2)
        xq = (x_pred.double() + 6e-8 * 0.3 * torch.randn(x_pred.shape, generator=g, dtype=torch.float64)).requires_grad_(True)
        sl.double()(xq, x_true.double()).backward()
        dq = xq.grad - xp.grad
        c_l2, c_max = float(dq.norm() / xp.grad.norm()), float(dq.abs().max() / xp.grad.abs().max())
        y_l2, y_max = max(y_l2, c_l2), max(y_max, c_max)
        # framing pair (+ library rfft) against torch.stft, value and gradient
        xa = x_pred.cuda().requires_grad_(True)
        xb = x_pred.cuda().requires_grad_(True)
        fa = sl_gpu.stft_ri(xa)
        fb = torch.view_as_real(sl_gpu.stft(xb)).transpose(1, 2)
        w = torch.randn(fa.shape, generator=g).cuda()
        (fa * w).sum().backward()
        (fb * w).sum().backward()
        e_fr = float((fa - fb).abs().max() / fb.abs().max())
        e_frg = float((xa.grad - xb.grad).abs().max() / xb.grad.abs().max())
        # column sums
        M, N = int(rng.integers(0, 20000)), int(rng.integers(1, 1600))
        dt = [torch.float32, torch.bfloat16, torch.float16][int(rng.integers(0, 3))]
        xm = torch.randn(M, N, generator=g).cuda().to(dt)
        e_cs = float((dense.colsum(xm).double() - xm.double().sum(0)).abs().max()) / max(1.0, float(xm.double().abs().sum(0).max())) if M else \
            float(dense.colsum(xm).abs().max())
        # (1e-3: single-frame cases -- a signal barely longer than the padding -- scatter between 2e-6 and 1e-3 for the round-2
        #  kernels, the round-3 kernels and torch's own fp32 formulation alike, dominated by the near-empty bins: measured with
        #  tools/microbench/mss_case.py)
        ratios.append(e_l2 / max(y_l2, 1e-7))
        okay = (fused and e_loss <= 2e-5 and e_l2 <= max(1e-3, 8.0 * y_l2) and e_max <= max(2e-3, 8.0 * y_max)
                and e_fr <= 3e-6 and e_frg <= 3e-6 and e_cs <= 2e-6)
        bad += not okay
        if verbose or not okay:
            print(f"{'ok ' if okay else 'BAD'} case {i}: n_fft {n_fft} overlap {overlap} B {B} L {L} | loss {e_loss:.1e} grad L2 {e_l2:.1e} (fp32 torch {y_l2:.1e}) max {e_max:.1e} ({y_max:.1e}) | "
                  f"frames {e_fr:.1e} grad {e_frg:.1e} | colsum [{M},{N}] {str(dt)[6:]} {e_cs:.1e}")
    r = np.array(ratios)
    print(f"gradient error / yardstick (the larger of torch fp32's own error and the fp32-epsilon conditioning probe): geometric mean "
          f"{float(np.exp(np.log(np.maximum(r, 1e-12)).mean())):.2f}, 90th percentile {float(np.percentile(r, 90)):.2f}, worst {float(r.max()):.2f}")
    return bad


def sweep_encoder_stages(cases: int, seed: int, verbose: bool = True):
    """Random cases of the encoder's loudness and resampler kernels (R_enc.sweep_cases: random n_fft / hop / frame count with every
    hop-long segment at its own level over six decades, random rate pair and length) against the fp64 references of
    tests/encoder_reference.py, at the tests' tolerances: loudness 2e-6, resampled audio 1e-6.  -> (failed, {stage: worst error})"""
    worst = {"loudness": 0.0, "resample": 0.0}
    bad = 0
    for i, c in enumerate(R_enc.sweep_cases(cases, seed)):
        x = torch.from_numpy(c["x"]).cuda()
        if c["kind"] == "loudness":
            got = R_enc.loudness_encoder(c["n_fft"], c["hop"]).cuda()(x).cpu().numpy()[..., 0]
            ref = R_enc.loudness_ref(c["x"], c["n_fft"], c["hop"], R_enc.a_weight_of(c["n_fft"]))
            tol, what = R_enc.LOUDNESS_TOL, f"n_fft {c['n_fft']} hop {c['hop']} [{x.shape[0]}, {ref.shape[1]}] frames"
        else:
            got = ddsp.encoder.Resample(c["orig"], c["new"]).cuda()(x).cpu().numpy()
            ref = R_enc.resample_ref(c["x"], c["orig"], c["new"])
            tol, what = R_enc.RESAMPLE_TOL, f"{c['orig']} -> {c['new']} [{x.shape[0]}, {x.shape[1]}]"
        err = float(np.abs(got - ref).max()) if got.shape == ref.shape else float("inf")
        okay = err <= tol                                        # a NaN fails
        bad += not okay
        worst[c["kind"]] = max(worst[c["kind"]], err) if okay or err == err else float("nan")
        if verbose or not okay:
            print(f"{'ok ' if okay else 'BAD'} case {i}: {c['kind']} {what}: {err:.2e}", flush=True)
    return bad, worst


def sweep_griffinlim_stages(cases: int, seed: int, verbose: bool = True):
    """Random cases of Griffin-Lim's three kernels, each alone through ddsp_griffinlim_stage (R_gl.random_case: random n_fft, hop
    up to n_fft / 2 with a Hann window of random win_length and up to n_fft with the rectangular one, B, T <= 40, extra length, c,
    with and without initial angles, R and Rprev), under the criteria of the stages alone: synthesis and analysis at most
    CPU_FACTOR times the CPU fp32 formulation's error and under the derived ceiling, the overlap-add bit for bit the fp32
    restatement and within the summation bound.  -> (failed, the figures of the failed cases)"""
    rng = np.random.default_rng(seed)
    bad, report = 0, []
    for i in range(cases):
        case = R_gl.random_case(rng)
        okay, lines = R_gl.run_case(case, seed * 1000 + i)
        bad += not okay
        if verbose or not okay:
            print(f"{'ok ' if okay else 'BAD'} case {i}: {case}\n  " + "\n  ".join(lines), flush=True)
        if not okay:
            report.extend(lines)
    return bad, report


def sweep_mss_stages(cases: int, seed: int, verbose: bool = True):
    """Random cases of ONE spectral-loss scale through ddsp_mss_scale directly (R_mss.random_case: random n_fft, hop 1 .. n_fft, B, L,
    alpha, eps and, in half the cases, hop-long segments at their own levels) under the criteria of tests/mss_reference.py: every
    bin of every frame of the gradient spectrum within its derived bound (or CPU_FACTOR times the stock fp32 formulation's error),
    undecided bins against the candidate signs and at most 0.5 % of a case's bins, lin and log each within 2e-5, the same three
    floats without grad_frames.  -> (failed, worst error / bound)"""
    rng = np.random.default_rng(seed)
    bad, worst = 0, 0.0
    for i in range(cases):
        case = R_mss.random_case(rng)
        xp, xt = R_mss.case_inputs(case)
        lines = []
        okay, w, _, _ = R_mss.run_case(xp, xt, case["n_fft"], case["hop"], case["alpha"], case["eps"], f"case {i}", lines)
        bad += not okay
        worst = max(worst, w)
        if verbose or not okay:
            print(f"{'ok ' if okay else 'BAD'} case {i}: {case}\n  " + "\n  ".join(lines), flush=True)
    return bad, worst


def main():
    cases = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 2026
    if len(sys.argv) > 3 and sys.argv[3] == "mss":
        bad, worst = sweep_mss_stages(cases, seed, verbose=True)
        print(f"spectral-loss scale, bin by bin: cases {cases}, seed {seed}, failed {bad}, worst error / bound {worst:.3f}")
        sys.exit(1 if bad else 0)
    if len(sys.argv) > 3 and sys.argv[3] == "griffinlim":
        bad, _ = sweep_griffinlim_stages(cases, seed, verbose=True)
        print(f"Griffin-Lim stages: cases {cases}, seed {seed}, failed {bad}")
        sys.exit(1 if bad else 0)
    if len(sys.argv) > 3 and sys.argv[3] == "chunked":
        bad, worst = sweep_chunked(cases, seed, verbose=False)
        print(f"chunked oscillator form: cases {cases}, seed {seed}, failed {bad}, worst audio error {worst:.2e}")
        sys.exit(1 if bad else 0)
    if len(sys.argv) > 3 and sys.argv[3] == "backward":
        bad, worst = sweep_osc_backward(cases, seed, verbose=False)
        print(f"oscillator backward: cases {cases}, seed {seed}, failed {bad}; worst error / yardstick per family: "
              + ", ".join(f"{k} {v:.1e}" for k, v in sorted(worst.items())))
        sys.exit(1 if bad else 0)
    if len(sys.argv) > 3 and sys.argv[3] == "noise_backward":
        bad, worst = sweep_noise_backward(cases, seed, verbose=False)
        print(f"noise backward: cases {cases}, seed {seed}, failed {bad}; worst error / yardstick per form: "
              + ", ".join(f"{k} {v:.1e}" for k, v in sorted(worst.items())))
        sys.exit(1 if bad else 0)
    if len(sys.argv) > 3 and sys.argv[3] == "noise_forward":
        bad, worst = sweep_noise_forward(cases, seed, verbose=False)
        print(f"noise forward: cases {cases}, seed {seed}, failed {bad}; worst error / yardstick per form: "
              + ", ".join(f"{k} {v:.1e}" for k, v in sorted(worst.items())))
        sys.exit(1 if bad else 0)
    if len(sys.argv) > 3 and sys.argv[3] == "gru":
        counts = {}
        bad, worst = sweep_gru(cases, seed, verbose=False, counts=counts)
        print(f"GRU recurrence: cases {cases}, seed {seed}, failed {bad}; worst error / e32 per family: "
              + ", ".join(f"{k} {v:.2f}" for k, v in sorted(worst.items())) + "; instantiations reached: "
              + ", ".join(f"{k} x{v}" for k, v in sorted(counts.items())))
        sys.exit(1 if bad else 0)
    if len(sys.argv) > 3 and sys.argv[3] == "encoder":
        bad, worst = sweep_encoder_stages(cases, seed, verbose=False)
        print(f"encoder stages: cases {cases}, seed {seed}, failed {bad}; worst error: "
              + ", ".join(f"{k} {v:.2e}" for k, v in sorted(worst.items())))
        sys.exit(1 if bad else 0)
    if len(sys.argv) > 3 and sys.argv[3] == "training":
        bad = sweep_training_kernels(cases, seed, verbose=False)
        print(f"loss-side kernels (one-kernel spectral scales, framing, column sums): cases {cases}, seed {seed}, failed {bad}")
        sys.exit(1 if bad else 0)
    bad, worst_osc, worst_noise = sweep(cases, seed)
    print(f"cases {cases}, failed {bad}, worst audio error {worst_osc:.2e}, worst noise error {worst_noise:.2e}")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
