#!/usr/bin/env python
"""Times the wavetable synthesiser (wavetable.py) at the 16 kHz training shape: B = 512 clips of T = 500 frames
of hop 128, N in {16, 32} tables of L = 512 points -- the forward and forward + backward of the HIP kernels in both forms (the
tables staged in LDS / read from memory, forced through ddsp_wavetable_set_form), beside
  * the same definition written with torch operations (upsample, cumsum in fp64, two gathers, the mix) on the same device, and
  * `OscillatorBank` at n_harmonics = 100 on the same f0 and loudness.
Device events on the stream, warm-up first, `--repeats` timings each of as many calls as fill `--window` seconds (counted from a
probe of the call, so a 0.4 ms kernel is timed over hundreds of calls) and the whole measurement `--runs` times, the forms
alternating inside a run: the median, the smallest and the largest of each timing are printed in one JSON line.  At the timed size
the tool also holds `--check-rows` rows of the HIP forward (both forms), of the HIP gradients and of the torch-op forward against
the fp64 reference of tests/wavetable_reference.py (error over its bound), and the device's fp32 `F.interpolate` of the increments
against the definition's -- the difference that makes the torch-op form's phase drift.  There is no threshold: DESIGN.md section 5b
records the figures.  The one claim it checks is printed as `hip_forward_faster_than_torch_ops`.

Band-limited rows, beside the unlimited ones in the same run: `bl_*_forward` (the cached pyramid, one launch),
`bl_*_forward_backward` (mip build, synthesis, its backward, the adjoint) and `mip_build` alone; `planned` lets a unit stage the
levels it hears when they fit, `global` reads them from memory.  Two f0 tracks: the tool's random one (every row hears five levels:
no row fits) and `notes` (a note per row with a vibrato of +-50 cents: a row hears two or three levels).  `bl_rows_that_stage` is
the share of rows whose levels fit -- the share of units at batches of 256 rows and more, where a row is one unit.

    python tools/bench_wavetable.py [--batch 512] [--frames 500] [--hop 128] [--tables 16 32] [--size 512] [--window 0.25] [--repeats 5] [--runs 2] [--check-rows 2]
"""
import argparse
import json
import os
import statistics
import sys

os.environ.setdefault("DDSP_TEST_HOOKS", "1")      # the form hook; read when the library is loaded

import torch                                       # noqa: E402
import torch.nn.functional as F                    # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import ddsp_pytorch_amd as ddsp                    # noqa: E402
import wavetable_reference as ref                  # noqa: E402

RATE = 16000
WINDOW = 0.25


def timed(fn, warmup, repeats):
    """-> (median ms per call over `repeats` timings, their smallest and largest); each timing runs the call back to back for about
    WINDOW seconds (the count comes from a probe after the warm-up)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()

    def window(iters):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(iters):
            fn()
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop) / iters
    iters = max(3, int(WINDOW * 1e3 / max(window(3), 1e-3)))
    ms = [window(iters) for _ in range(repeats)]
    return statistics.median(ms), min(ms), max(ms), iters


def check_against_fp64(f0, c, a, W, gy, hop, rows, lib):
    """The rows `rows` of the timed batch against the fp64 reference: error over bound of the HIP forms and of the torch-op form."""
    import numpy as np
    host = lambda x: x.detach()[rows].cpu().numpy()                             # noqa: E731
    f0h, ch, ah, Wh, gyh = host(f0)[..., 0], host(c), host(a)[..., 0], W.detach().cpu().numpy(), host(gy).astype(np.float64)
    want, bound, _ = ref.forward(f0h, ch, ah, Wh, hop, RATE)
    over = lambda got, w, b: float((np.abs(got.cpu().numpy().astype(np.float64) - w) / np.maximum(b, 1e-300)).max())   # noqa: E731
    out = {}
    sub = (f0[rows].contiguous(), c.detach()[rows].contiguous(), a.detach()[rows].contiguous())
    g = ref.backward(gyh, f0h, ch, ah, Wh, hop, RATE)
    for name, mode in (("lds", 1), ("global", 2)):
        assert lib.ddsp_wavetable_set_form(mode) == 0
        if lib.ddsp_wavetable_form(len(rows), f0.shape[1], c.shape[2], W.shape[1], hop) < 0:
            continue
        out[f"hip_{name}_forward_err_over_bound"] = over(ddsp.wavetable_forward(*sub, W.detach(), hop, RATE), want, bound)
        grads = ddsp.wavetable_backward(gy[rows].contiguous(), *sub, W.detach(), hop, RATE)
        for key, got in zip(("c", "a", "W"), grads):
            out[f"hip_{name}_grad_{key}_err_over_bound"] = over(got, g["grad_" + key], g["bound_" + key])
    assert lib.ddsp_wavetable_set_form(0) == 0
    with torch.no_grad():
        yt = torch_ops_forward(*sub, W.detach(), hop)
        up_dev = F.interpolate((sub[0] / RATE).transpose(1, 2), scale_factor=hop, mode="linear", align_corners=False)[:, 0]
    out["torch_ops_forward_err_over_bound"] = over(yt, want, bound)
    out["torch_ops_forward_max_abs_err"] = float(np.abs(yt.cpu().numpy().astype(np.float64) - want).max())
    u = ref.increments(f0h, hop, RATE)
    du = up_dev.cpu().numpy().astype(np.float64) - u
    out["device_interpolate_vs_definition"] = dict(samples_that_differ=float((du != 0).mean()), max_abs=float(np.abs(du).max()),
                                                   phase_drift_cycles=float(np.abs(np.cumsum(du, 1)).max()))
    return out


def rows_that_stage(f0, L, fit):
    """Share of rows whose frames hear at most `fit` levels, by the kernel's rule (g = f0 / sample_rate widened by 2^-20)."""
    g = (f0[..., 0] / RATE).float()

    def level(u):
        r = (u * L).double()
        q = torch.where(r > 0.5, torch.frexp(r.clamp(min=0.5))[1].double(), torch.zeros_like(r))
        return torch.where(r >= L / 2, torch.full_like(r, L.bit_length() - 1), q)
    lo = level(g * (1.0 - 2.0 ** -20)).amin(1)
    hi = (level(g * (1.0 + 2.0 ** -20)) + 1).clamp(max=L.bit_length() - 1).amax(1)
    return float(((hi - lo + 1) <= fit).double().mean())


def torch_ops_forward(f0, c, a, W, hop):
    """The definition of section 5b as torch operations (fp32, the phase in fp64)."""
    up = lambda x: F.interpolate(x.transpose(1, 2), scale_factor=hop, mode="linear", align_corners=False).transpose(1, 2)   # noqa: E731
    L = W.shape[1]
    P = torch.cumsum(up(f0 / RATE)[..., 0].double(), 1)
    pos = (P - P.floor()) * L
    j = pos.floor().long().clamp_(0, L - 1)
    fr = (pos - j).float()
    Wt = W.t()                                                                  # [L, N]: one gathered row per sample
    lo, hi = Wt[j], Wt[(j + 1) % L]
    s = lo + fr[..., None] * (hi - lo)
    wn = c / c.sum(-1, keepdim=True)
    return up(a)[..., 0] * (up(wn) * s).sum(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--frames", type=int, default=500)
    ap.add_argument("--hop", type=int, default=128)
    ap.add_argument("--tables", type=int, nargs="+", default=[16, 32])
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--window", type=float, default=WINDOW)
    ap.add_argument("--check-rows", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--no-band-limited", action="store_true", help="leave the band-limited rows out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_wavetable.py measures on the GPU; none is visible")
    dev = torch.device("cuda")
    globals()["WINDOW"] = args.window
    B, T, hop, L = args.batch, args.frames, args.hop, args.size
    lib = ddsp._lib.lib()
    g = torch.Generator(device="cuda").manual_seed(0)
    f0 = 80.0 + 700.0 * torch.rand((B, T, 1), device=dev, generator=g)
    a = 0.1 + torch.rand((B, T, 1), device=dev, generator=g)
    # `notes`: a note per row in the same range, with a 5 Hz vibrato of +-50 cents
    note = 80.0 * (780.0 / 80.0) ** torch.rand((B, 1, 1), device=dev, generator=g)
    f0_notes = note * 2.0 ** (torch.sin(2.0 * torch.pi * 5.0 * hop / RATE * torch.arange(T, device=dev).view(1, T, 1)) / 24.0)
    gy = torch.randn((B, T * hop), device=dev, generator=g)
    samples = B * T * hop
    results = {}

    class BankConf:
        n_harmonics, sample_rate, hop_length = 100, RATE, hop
    bank = ddsp.OscillatorBank(BankConf).to(dev)
    cb = (0.05 + torch.rand((B, T, 100), device=dev, generator=g)).requires_grad_()
    ab = a.clone().requires_grad_()

    def bank_step():
        y = bank({"f0": f0, "c": cb, "a": ab})
        y.backward(gy)
        cb.grad = ab.grad = None
        return y

    for N in args.tables:
        class Conf:
            n_harmonics, sample_rate, hop_length = N, RATE, hop
        wt = ddsp.WavetableBank(Conf, table_size=L, init=torch.randn((N, L), generator=torch.Generator().manual_seed(N))).to(dev)
        c = (0.05 + torch.rand((B, T, N), device=dev, generator=g)).requires_grad_()
        aw = a.clone().requires_grad_()
        x = {"f0": f0, "c": c, "a": aw}

        def forward():
            with torch.no_grad():
                return wt(x)

        def step():
            y = wt(x)
            y.backward(gy)
            c.grad = aw.grad = wt.wavetables.grad = None
            return y

        def torch_forward():
            with torch.no_grad():
                return torch_ops_forward(f0, c, aw, wt.wavetables, hop)

        def torch_step():
            y = torch_ops_forward(f0, c, aw, wt.wavetables, hop)
            y.backward(gy)
            c.grad = aw.grad = wt.wavetables.grad = None
            return y

        bl, bl_info = None, {}
        if not args.no_band_limited:
            bl = ddsp.WavetableBank(Conf, table_size=L, init=wt.wavetables.detach().cpu(), band_limited=True).to(dev)
            plan = ddsp.wavetable_form_bl(B, T, N, L, hop)
            bl_info = dict(bl_planned=plan, bl_backward_scratch_bytes=int(lib.ddsp_wavetable_backward_bl_scratch_bytes(B, T, N, L, hop)),
                           bl_rows_that_stage=dict(forward=rows_that_stage(f0, L, plan["forward_fit"]),
                                                   backward=rows_that_stage(f0, L, plan["backward_fit"]),
                                                   forward_notes=rows_that_stage(f0_notes, L, plan["forward_fit"]),
                                                   backward_notes=rows_that_stage(f0_notes, L, plan["backward_fit"])))
        runs = []
        for _ in range(args.runs):
            t = {}
            for name, mode in (("lds", 1), ("global", 2)):
                assert lib.ddsp_wavetable_set_form(mode) == 0
                if lib.ddsp_wavetable_form(B, T, N, L, hop) > 0:                # (the LDS form may not fit: then it is not timed)
                    t[f"hip_{name}_forward"] = timed(forward, 3, args.repeats)
                if lib.ddsp_wavetable_form(B, T, N, L, hop) > 0:
                    t[f"hip_{name}_forward_backward"] = timed(step, 3, args.repeats)
            assert lib.ddsp_wavetable_set_form(0) == 0
            t["hip_planned_forward"] = timed(forward, 3, args.repeats)
            t["hip_planned_forward_backward"] = timed(step, 3, args.repeats)
            t["torch_ops_forward"] = timed(torch_forward, 2, args.repeats)
            t["torch_ops_forward_backward"] = timed(torch_step, 2, args.repeats)
            if bl is not None:
                for track, f in (("", f0), ("_notes", f0_notes)):
                    xb = {"f0": f, "c": c, "a": aw}

                    def bl_forward():
                        with torch.no_grad():
                            return bl(xb)

                    def bl_step():
                        y = bl(xb)
                        y.backward(gy)
                        c.grad = aw.grad = bl.wavetables.grad = None
                        return y
                    for name, mode in (("planned", 0), ("global", 2)):
                        assert lib.ddsp_wavetable_set_form(mode) == 0
                        t[f"bl_{name}_forward{track}"] = timed(bl_forward, 3, args.repeats)
                        t[f"bl_{name}_forward_backward{track}"] = timed(bl_step, 3, args.repeats)
                    assert lib.ddsp_wavetable_set_form(0) == 0
                t["mip_build"] = timed(lambda: ddsp.wavetable_mipmaps(bl.wavetables.detach()), 3, args.repeats)
            if N == args.tables[0]:
                t["bank100_forward"] = timed(lambda: bank({"f0": f0, "c": cb.detach(), "a": ab.detach()}), 3, args.repeats)
                t["bank100_forward_backward"] = timed(bank_step, 3, args.repeats)
            runs.append({k + "_ms": [round(v, 4) for v in t[k][:3]] + [t[k][3]] for k in t})      # median, smallest, largest, calls
        med = lambda key: statistics.median(r[key][0] for r in runs)            # noqa: E731
        rows = sorted({int(r) for r in torch.linspace(0, B - 1, max(args.check_rows, 1))}) if args.check_rows > 0 else []
        checks = check_against_fp64(f0, c, aw, wt.wavetables, gy, hop, rows, lib) if rows else {}
        form = ddsp.wavetable_form(B, T, N, L, hop)
        results[f"N{N}"] = dict(
            planned=form, rows_checked_against_fp64=rows, **checks, **bl_info,
            hip_forward_Msamples_per_s=round(samples / med("hip_planned_forward_ms") / 1e3, 1),
            hip_forward_faster_than_torch_ops=bool(med("hip_planned_forward_ms") < med("torch_ops_forward_ms")),
            torch_ops_over_hip_forward=round(med("torch_ops_forward_ms") / med("hip_planned_forward_ms"), 2),
            torch_ops_over_hip_forward_backward=round(med("torch_ops_forward_backward_ms") / med("hip_planned_forward_backward_ms"), 2),
            median_smallest_largest_per_run=runs)
    print(json.dumps(dict(shape=dict(batch=B, frames=T, hop=hop, table_size=L, sample_rate=RATE, samples=samples),
                          window_s=args.window, repeats=args.repeats, results=results)))


if __name__ == "__main__":
    main()
