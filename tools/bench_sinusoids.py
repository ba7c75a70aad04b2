#!/usr/bin/env python
"""Times the inharmonic sinusoid bank (sinusoids.py) at the 16 kHz training shape: B = 512 clips of T = 500
frames of hop 128, K = 100 partials -- the HIP forward, and forward + backward with and without grad_f -- beside
  * the same definition written with torch operations (fp64 upsampling and cumsum of the increments, sin, the mix) on the same
    device, run over slices of `--torch-rows` rows because its [rows, T hop, K] intermediates do not fit otherwise, and
  * `OscillatorBank` at n_harmonics = 100 on the same f0, weights and loudness.
Every GPU step is a child process of this tool under its own time limit; the parent never opens the device, checks every exit
status and starts nothing more after a step that failed.  Device events on the stream, warm-up first, `--repeats` timings each of
as many calls as fill `--window` seconds, the whole measurement `--runs` times: the median, the smallest and the largest of each
timing are printed in one JSON line.  The `check` step holds rows 0 and B - 1 of the timed batch -- forward and the three gradients
-- against the fp64 reference of tests/sinusoids_reference.py as a fraction of their bounds.  There is no threshold: DESIGN.md
section 5d records the figures.  The one claim it checks is printed as `hip_faster_than_torch_ops`.

    python tools/bench_sinusoids.py [--batch 512] [--frames 500] [--hop 128] [--partials 100] [--window 0.25] [--repeats 5] [--runs 2]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATE = 16000
STEPS = {"hip": 240, "bank": 120, "torch": 420, "check": 420}       # seconds each step may take


def timed(torch, fn, warmup, repeats, window_s):
    """-> [median ms per call over `repeats` timings, their smallest, their largest, calls per timing]"""
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
    iters = max(3, int(window_s * 1e3 / max(window(3), 1e-3)))
    ms = [window(iters) for _ in range(repeats)]
    return [round(statistics.median(ms), 4), round(min(ms), 4), round(max(ms), 4), iters]


def torch_ops_forward(torch, F, f, c, a, hop):
    """The definition of section 5d as torch operations: the phase as the fp64 running sum of the upsampled increments."""
    up = lambda x: F.interpolate(x.transpose(1, 2), scale_factor=hop, mode="linear", align_corners=False).transpose(1, 2)   # noqa: E731
    valid = torch.isfinite(f) & (f >= 0)
    g = torch.where(valid, f.double() / RATE, torch.zeros((), dtype=torch.float64, device=f.device))
    w = torch.where(valid & ~(f > RATE // 2), c, torch.zeros((), device=f.device))
    S = w.sum(-1, keepdim=True)
    wn = torch.where(S != 0, w / S, torch.zeros((), device=f.device))
    P = torch.cumsum(up(g), 1)
    s = torch.sin(2.0 * torch.pi * (P - P.floor())).float()
    return up(a)[..., 0] * (up(wn) * s).sum(-1)


def child(args):
    import numpy as np
    import torch
    import torch.nn.functional as F
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import ddsp_pytorch_amd as ddsp
    if not torch.cuda.is_available():
        raise SystemExit("bench_sinusoids.py measures on the GPU; none is visible")
    dev = torch.device("cuda")
    B, T, hop, K = args.batch, args.frames, args.hop, args.partials
    g = torch.Generator(device="cuda").manual_seed(0)
    f0 = 60.0 + 400.0 * torch.rand((B, T, 1), device=dev, generator=g)
    a = 0.1 + torch.rand((B, T, 1), device=dev, generator=g)
    c = 0.05 + torch.rand((B, T, K), device=dev, generator=g)
    gy = torch.randn((B, T * hop), device=dev, generator=g)

    class Conf:
        n_harmonics, sample_rate, hop_length = K, RATE, hop
    inh = ddsp.InharmonicBank(Conf, inharmonicity=1e-4).to(dev)        # a stiff string: partial 100 sits at 141 f0
    fixed = ddsp.InharmonicBank(Conf, inharmonicity=1e-4, learn=False).to(dev)
    cg, ag = c.clone().requires_grad_(), a.clone().requires_grad_()
    x, xg = {"f0": f0, "c": c, "a": a}, {"f0": f0, "c": cg, "a": ag}
    out = {}
    run = lambda fn, warm=3: timed(torch, fn, warm, args.repeats, args.window)          # noqa: E731

    def step_of(module):
        def step():
            y = module(xg)
            y.backward(gy)
            cg.grad = ag.grad = None
            for p in module.parameters():
                p.grad = None
        return step

    def module_forward():
        with torch.no_grad():
            return inh(x)

    if args.step == "hip":
        lib = ddsp._lib.lib()
        out["forward_scratch_bytes"] = int(lib.ddsp_sinusoids_scratch_bytes(B, T, K, hop))
        out["backward_scratch_bytes"] = dict(with_grad_f=int(lib.ddsp_sinusoids_backward_scratch_bytes(B, T, K, hop, 1)),
                                             without=int(lib.ddsp_sinusoids_backward_scratch_bytes(B, T, K, hop, 0)))
        with torch.no_grad():
            f = inh.frequencies(x).contiguous()
        out["masked_share"] = float((f > RATE // 2).float().mean())
        out["runs"] = []
        for _ in range(args.runs):
            out["runs"].append(dict(
                hip_forward_ms=run(lambda: ddsp.sinusoids_forward(f, c, a, hop, RATE)),
                hip_module_forward_ms=run(module_forward),
                hip_forward_backward_grad_f_ms=run(step_of(inh)),
                hip_forward_backward_fixed_ms=run(step_of(fixed))))
    elif args.step == "bank":
        bank = ddsp.OscillatorBank(Conf).to(dev)
        out["runs"] = []
        for _ in range(args.runs):
            out["runs"].append(dict(bank100_forward_ms=run(lambda: bank(x)), bank100_forward_backward_ms=run(step_of(bank))))
    elif args.step == "torch":
        R = args.torch_rows
        with torch.no_grad():
            f = inh.frequencies(x).contiguous()

        def torch_forward():
            with torch.no_grad():
                for r in range(0, B, R):
                    torch_ops_forward(torch, F, f[r:r + R], c[r:r + R], a[r:r + R], hop)

        def torch_step():
            for r in range(0, B, R):
                fs = f[r:r + R].clone().requires_grad_()
                cs, as_ = c[r:r + R].clone().requires_grad_(), a[r:r + R].clone().requires_grad_()
                torch_ops_forward(torch, F, fs, cs, as_, hop).backward(gy[r:r + R])
        out["torch_rows_per_slice"] = R
        out["runs"] = [dict(torch_ops_forward_ms=timed(torch, torch_forward, 1, 3, 0.0), torch_ops_forward_backward_ms=timed(torch, torch_step, 1, 3, 0.0))]
    elif args.step == "check":
        import sinusoids_reference as ref
        rows = sorted({0, B - 1})
        with torch.no_grad():
            f = inh.frequencies(x)[rows].contiguous()
        sub = (f, c[rows].contiguous(), a[rows].contiguous())
        fh, ch, ah, gyh = (t.cpu().numpy() for t in sub + (gy[rows],))
        want = ref.forward(fh, ch, ah, hop, RATE)
        over = lambda got, w, b: float((np.abs(got.cpu().numpy().astype(np.float64) - w) / np.maximum(b, 1e-300)).max())   # noqa: E731
        out["rows"] = rows
        out["hip_forward_err_over_bound"] = over(ddsp.sinusoids_forward(*sub, hop, RATE), want["y"], want["bound"])
        wb = ref.backward(gyh.astype(np.float64), fh, ch, ah, hop, RATE)
        for key, got in zip(("f", "c", "a"), ddsp.sinusoids_backward(gy[rows].contiguous(), *sub, hop, RATE)):
            out[f"hip_grad_{key}_err_over_bound"] = over(got, wb["grad_" + key], wb["bound_" + key])
        with torch.no_grad():
            yt = torch_ops_forward(torch, F, *sub, hop)
        out["torch_ops_forward_err_over_bound"] = over(yt, want["y"], want["bound"])
        out["torch_ops_forward_max_abs_err"] = float(np.abs(yt.cpu().numpy().astype(np.float64) - want["y"]).max())
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--frames", type=int, default=500)
    ap.add_argument("--hop", type=int, default=128)
    ap.add_argument("--partials", type=int, default=100)
    ap.add_argument("--window", type=float, default=0.25)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--torch-rows", type=int, default=16)
    ap.add_argument("--steps", nargs="+", default=list(STEPS), choices=list(STEPS))
    ap.add_argument("--step", choices=list(STEPS), help=argparse.SUPPRESS)       # (a child of this tool)
    args = ap.parse_args()
    if args.step:
        return child(args)
    results = {}
    passed = sys.argv[1:]
    for name in args.steps:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name] + passed, capture_output=True, text=True,
                               timeout=STEPS[name])
        except subprocess.TimeoutExpired:
            print(json.dumps(dict(failed=name, reason=f"no result within {STEPS[name]} s", results=results)))
            raise SystemExit(f"bench_sinusoids.py: step {name} ran past its limit of {STEPS[name]} s; nothing more is started")
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not lines:
            print(json.dumps(dict(failed=name, returncode=r.returncode, stderr=r.stderr[-2000:], results=results)))
            raise SystemExit(f"bench_sinusoids.py: step {name} ended with status {r.returncode}; nothing more is started")
        results[name] = json.loads(lines[-1][len("RESULT "):])
    med = lambda step, key: statistics.median(run[key][0] for run in results[step]["runs"])     # noqa: E731
    summary = {}
    if "hip" in results and "torch" in results:
        summary["torch_ops_over_hip_forward"] = round(med("torch", "torch_ops_forward_ms") / med("hip", "hip_forward_ms"), 1)
        summary["torch_ops_over_hip_forward_backward"] = round(med("torch", "torch_ops_forward_backward_ms")
                                                                / med("hip", "hip_forward_backward_grad_f_ms"), 1)
        summary["hip_faster_than_torch_ops"] = bool(summary["torch_ops_over_hip_forward"] > 1 and summary["torch_ops_over_hip_forward_backward"] > 1)
    if "hip" in results and "bank" in results:
        summary["hip_over_bank100_forward"] = round(med("hip", "hip_forward_ms") / med("bank", "bank100_forward_ms"), 2)
        summary["hip_over_bank100_forward_backward"] = round(med("hip", "hip_forward_backward_grad_f_ms") / med("bank", "bank100_forward_backward_ms"), 2)
    print(json.dumps(dict(shape=dict(batch=args.batch, frames=args.frames, hop=args.hop, partials=args.partials, sample_rate=RATE,
                                     samples=args.batch * args.frames * args.hop),
                          window_s=args.window, repeats=args.repeats, summary=summary, results=results)))


if __name__ == "__main__":
    main()
