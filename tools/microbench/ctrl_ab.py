"""Same-box A/B of two libddsp_hip.so builds on the controller's LayerNorm + LeakyReLU passes (csrc/ddsp_ctrl.hip):

    python tools/microbench/ctrl_ab.py PARENT.so NEW.so --out profiles/ctrl_refactor_ab.json [--train-step]

Part one, bits: from seeded inputs, at the row counts where the kernels take another path and every (D, type) the entries accept,
the SHA-256 of every output tensor; the two libraries' digest lists must be identical.  Part two, time: five rounds, the library that
runs first alternating by round, at the training shape (16 000 rows, D = 512), microseconds per call between device events after a
warm-up; every new median must lie within the parent's median plus the parent's own spread (max - min over its rounds).
--train-step adds bench.py's training step (fp16 + GradScaler, bf16) from one run on each library, for the record.

One child process per library and round (DDSP_HIP_LIB selects the library), one after the other, each under its own time limit; the
first child that fails ends the chain and the tool exits non-zero.  The entries are called through the C ABI on buffers allocated once,
so the timed loop holds nothing but the launches."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ROWS = (1, 3, 277, 4101)          # tests/test_decoder_training.py: _LN_ROWS
ROWS_FWD_ONLY = 16389             # the forward's grid-stride loop (4096 workgroups of four rows)
EPS, SLOPE = 1e-5, 0.01
TIMED_ROWS, TIMED_D = 16000, 512
ROUNDS = 5


def _passes(torch, L, dtype, D, rows, first_block):
    """-> (forward(), backward(), {name: output tensor}) of one configuration on buffers allocated here."""
    io = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}[dtype]
    dev = "cuda"
    f32 = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.float32)                    # noqa: E731
    gamma, beta = f32(D).uniform_(0.5, 1.5), f32(D).uniform_(-0.3, 0.3)
    gy = torch.randn(rows, D, device=dev).to(dtype)
    y, mean, rstd = torch.empty(rows, D, device=dev, dtype=dtype), f32(rows), f32(rows)
    stream = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()                                                                  # noqa: E731

    def check(rc):
        if rc != 0:
            raise RuntimeError(f"return code {rc} ({dtype}, D = {D}, rows = {rows}, first block: {first_block})")

    if first_block:
        xs, w, bias = f32(rows).uniform_(-1.0, 1.0), f32(D).uniform_(-1.0, 1.0), f32(D).uniform_(-1.0, 1.0)
        grads = f32(4, D)
        scratch = torch.empty(L.ddsp_outer_ln_lrelu_scratch_bytes(D), device=dev, dtype=torch.uint8)
        fwd, bwd = L.ddsp_outer_ln_lrelu_forward, L.ddsp_outer_ln_lrelu_backward
        fwd_args = (p(xs), p(w), p(bias), p(gamma), p(beta), p(y), p(mean), p(rstd), rows, D, EPS, SLOPE, io, stream)
        bwd_args = (p(gy), p(xs), p(w), p(bias), p(y), p(gamma), p(mean), p(rstd), p(grads[0]), p(grads[1]), p(grads[2]), p(grads[3]),
                    p(scratch), rows, D, SLOPE, io, stream)
        outs = {"y": y, "mean": mean, "rstd": rstd, "d_w": grads[0], "d_bias": grads[1], "d_gamma": grads[2], "d_beta": grads[3]}
    else:
        x = torch.randn(rows, D, device=dev).to(dtype)
        gx, grads = torch.empty_like(x), f32(3, D)
        scratch = torch.empty(L.ddsp_ln_lrelu_scratch_bytes(D), device=dev, dtype=torch.uint8)
        tail = () if io == 0 else (io,)
        fwd, bwd = (L.ddsp_ln_lrelu_forward, L.ddsp_ln_lrelu_backward) if io == 0 else (L.ddsp_ln_lrelu_forward_16, L.ddsp_ln_lrelu_backward_16)
        fwd_args = (p(x), p(gamma), p(beta), p(y), p(mean), p(rstd), rows, D, EPS, SLOPE, *tail, stream)
        bwd_args = (p(gy), p(x), p(y), p(gamma), p(mean), p(rstd), p(gx), p(grads[0]), p(grads[1]), p(grads[2]), p(scratch), rows, D, SLOPE,
                    *tail, stream)
        outs = {"y": y, "mean": mean, "rstd": rstd, "gx": gx, "d_gamma": grads[0], "d_beta": grads[1], "xsum": grads[2]}

    def forward():
        check(fwd(*fwd_args))

    def backward():
        check(bwd(*bwd_args))

    forward.inputs = (gamma, beta, gy, scratch) + ((xs, w, bias) if first_block else (x,))      # (the addresses above stay valid)
    return forward, backward, outs


def _child(part):
    import torch
    sys.path.insert(0, ROOT)
    import ddsp_pytorch_amd as ddsp
    L = ddsp._lib.lib()
    names = {torch.float32: "fp32", torch.bfloat16: "bf16", torch.float16: "fp16"}
    result = {}
    if part == "bits":
        sha = lambda t: hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()      # noqa: E731
        for first_block, widths in ((False, (256, 512, 768, 1024)), (True, (256, 512))):
            for D in widths:
                for dtype in names:
                    for rows in ROWS + (ROWS_FWD_ONLY,):
                        torch.manual_seed(1000 * D + rows)
                        forward, backward, outs = _passes(torch, L, dtype, D, rows, first_block)
                        forward()
                        if rows == ROWS_FWD_ONLY:
                            outs = {k: outs[k] for k in ("y", "mean", "rstd")}
                        else:
                            backward()
                        torch.cuda.synchronize()
                        for k, t in outs.items():
                            result[f"{'first_block' if first_block else 'layernorm'}/{names[dtype]}/D{D}/rows{rows}/{k}"] = sha(t)
    else:
        for first_block, dtypes in ((False, (torch.float32, torch.bfloat16, torch.float16)), (True, (torch.float32, torch.bfloat16))):
            for dtype in dtypes:
                torch.manual_seed(7)
                forward, backward, _ = _passes(torch, L, dtype, TIMED_D, TIMED_ROWS, first_block)
                for which, call in (("fwd", forward), ("bwd", backward)):      # (forward first: the backward reads its y / mean / rstd)
                    for _ in range(50):
                        call()
                    torch.cuda.synchronize()
                    blocks = []
                    for _ in range(5):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(200):
                            call()
                        e1.record()
                        torch.cuda.synchronize()
                        blocks.append(1e3 * e0.elapsed_time(e1) / 200)
                    result[f"{'first_block' if first_block else 'layernorm'}_{which}_{names[dtype]}"] = round(statistics.median(blocks), 3)
    print(json.dumps(result))


def _run(lib, argv, limit):
    """One child on one library under its own time limit -> the JSON object on its last output line."""
    env = dict(os.environ, DDSP_HIP_LIB=os.path.abspath(lib))
    r = subprocess.run([sys.executable] + argv, env=env, cwd=ROOT, capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"ctrl_ab: {' '.join(argv)} on {lib} ended with status {r.returncode}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("libs", nargs="*", metavar="LIB", help="the parent's library, then the new one")
    ap.add_argument("--out", help="the report (JSON)")
    ap.add_argument("--train-step", action="store_true", help="also one bench.py --mode train run (fp16, bf16) on each library")
    ap.add_argument("--child", choices=["bits", "time"], help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return _child(args.child)
    if len(args.libs) != 2 or not args.out:
        ap.error("two libraries and --out")
    libs = dict(zip(("parent", "new"), args.libs))
    me = os.path.abspath(__file__)
    report = {"what": "controller LayerNorm + LeakyReLU passes (ddsp_ln_lrelu_*, ddsp_outer_ln_lrelu_*), the library of the parent commit "
                      "against the new one: tools/microbench/ctrl_ab.py, one process per library and round, both libraries in one call "
                      "on one MI355X, selected with DDSP_HIP_LIB"}
    ok = True

    digests = {k: _run(lib, [me, "--child", "bits"], 300) for k, lib in libs.items()}
    differing = sorted(k for k in set(digests["parent"]) | set(digests["new"]) if digests["parent"].get(k) != digests["new"].get(k))
    report["bits"] = {"rows": list(ROWS) + [ROWS_FWD_ONLY], "digests": len(digests["new"]), "differing": differing,
                      "sha256_of_all_digests": hashlib.sha256(json.dumps(digests["new"], sort_keys=True).encode()).hexdigest()}
    print(f"bits: {len(digests['new'])} digests, {len(differing)} differ", flush=True)
    ok = ok and not differing and len(digests["new"]) > 0

    rounds = {k: [] for k in libs}
    for r in range(ROUNDS):
        for k in (("parent", "new") if r % 2 == 0 else ("new", "parent")):
            rounds[k].append(_run(libs[k], [me, "--child", "time"], 300))
            print(f"round {r + 1} {k}: {rounds[k][-1]}", flush=True)
    report["time"] = {"unit": "microseconds per call, one value per round (the median of five blocks of 200 calls)",
                      "shape": [TIMED_ROWS, TIMED_D], "order": f"{ROUNDS} rounds; odd rounds run parent then new, even rounds new then parent",
                      "entries": []}
    for name in rounds["parent"][0]:
        old, new = [r[name] for r in rounds["parent"]], [r[name] for r in rounds["new"]]
        bound = statistics.median(old) + (max(old) - min(old))
        within = statistics.median(new) <= bound
        report["time"]["entries"].append({"entry": name, "parent": old, "new": new, "parent_median": statistics.median(old),
                                          "new_median": statistics.median(new), "bound": round(bound, 3), "within": within})
        print(f"{name}: parent {statistics.median(old)} new {statistics.median(new)} bound {bound:.3f} {'ok' if within else 'SLOWER'}", flush=True)
        ok = ok and within

    if args.train_step:
        report["train_step_ms"] = {"what": "bench.py --gpus 1 --mode train --steps 30 --warmup 10, one run per library and type; for the record"}
        for amp in ("fp16", "bf16"):
            for k, lib in libs.items():
                line = _run(lib, ["bench.py", "--gpus", "1", "--mode", "train", "--amp", amp, "--steps", "30", "--warmup", "10"], 400)
                report["train_step_ms"][f"{amp}_{k}"] = round(line["ms_per_step"], 3)
                print(f"train step {amp} {k}: {line['ms_per_step']:.3f} ms", flush=True)

    report["verdict"] = "equal bits, every new median within the parent's median plus its spread" if ok else "FAILED"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
