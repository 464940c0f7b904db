"""Latency of the batched Burgers initial-condition stage (gmrf_bic_run) on burgers512x64, one process, one stream, batch 8 / 32 / 64.

Per batch size, medians of --reps after --warmup:
  ic_stage_ms           (a) `BurgersInitialConditionBatch.run` on device tensors: initial conditions -> bulk, prior values,
                        information vector -> refactor -> x_ic
  refactor_solve_ms     (b) `refactor` + `solve_batch` alone on the same handle and the same values, device tensors
  glue_ratio            (a) / (b)
  host_route_ms_per_problem
                        (c) the route the stage replaces: `workloads.burgers_gauss_newton_batch` for ONE problem on the host
                        (SciPy `bmat` and sparse products) plus the upload of a batch's q_values, Qx_prior, x_prior, x0 divided
                        by the batch
  host_over_device      (c) / ((a) / batch)
The batch repeats 8 distinct initial conditions.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t)


def measure(pkg, base_ics, host_ms, host_arrays, ns, nt, B, reps, warmup):
    import numpy as np
    import torch
    dt, nu, fem_noise = 1.0 / (nt - 1), 0.01 / np.pi, 1e12
    ics = np.ascontiguousarray(base_ics[np.arange(B) % base_ics.shape[0]])
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    prior = pkg.BurgersP1Prior(ns, nt, dt, nu, stream=s)
    tan = pkg.BurgersP1Tangent(ns, nt, dt, nu, stream=s)
    asm = pkg.PosteriorAssembler(prior.pattern, tan.pattern, stream=s)
    F = pkg.TridiagonalCholeskyFactor(stream=s, batch=B)
    d_ics = torch.from_numpy(ics).cuda()
    v = prior.values_batch(d_ics)
    x0 = v["bulk"][:, None].repeat(1, ns * nt).contiguous()
    jv, _ = tan.tangent_batch(x0)
    F.factor(asm.pattern, nt, values=asm.precision_batch(v["q_values"], jv, fem_noise).cpu().numpy())
    stage = pkg.BurgersInitialConditionBatch(F, asm, prior)
    r = {"batch": B}
    r["ic_stage_ms"] = _median_ms(lambda: stage.run(d_ics), reps, warmup)
    # (b): Q_ic's values in the assembler's order (J = 0, noise 0) and the same right-hand side, nothing else
    a = asm.precision_batch(v["q_values"], torch.zeros_like(jv), 0.0)
    rhs = v["Qx_prior"].reshape(B, 1, -1).contiguous()

    def refactor_solve():
        F.refactor(a)
        F.solve_batch(rhs)

    r["refactor_solve_ms"] = _median_ms(refactor_solve, reps, warmup)
    r["glue_ratio"] = r["ic_stage_ms"] / r["refactor_solve_ms"]
    # (c): one problem's host prior, and the upload of a batch of them
    idx = np.arange(B) % host_arrays["x0"].shape[0]
    up = [np.ascontiguousarray(host_arrays[k][idx]) for k in ("q_values", "Qx_prior", "x_prior", "x0")]

    def upload():
        for arr in up:
            torch.from_numpy(arr).cuda()
        torch.cuda.synchronize()

    r["upload_ms_per_problem"] = _median_ms(upload, reps, warmup) / B
    r["host_route_ms_per_problem"] = host_ms + r["upload_ms_per_problem"]
    r["device_ms_per_problem"] = r["ic_stage_ms"] / B
    r["host_over_device"] = r["host_route_ms_per_problem"] / r["device_ms_per_problem"]
    stage.close(); F.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batches", default="8,32,64")
    ap.add_argument("--ns", type=int, default=512)
    ap.add_argument("--nt", type=int, default=64)
    args = ap.parse_args()
    import numpy as np
    import __graft_entry__ as g
    pkg = g.load_package()
    W = pkg.workloads
    base_ics = W.burgers_initial_conditions(args.ns, 8) + 0.1 * np.arange(8)[:, None]          # (a bulk speed per problem)
    host_ms = _median_ms(lambda: W.burgers_gauss_newton_batch(args.ns, args.nt, 1), args.reps, args.warmup)
    host_arrays = W.burgers_gauss_newton_batch(args.ns, args.nt, 2)
    out = {"tool": "burgers_ic_latency", "workload": f"burgers{args.ns}x{args.nt}", "reps": args.reps, "warmup": args.warmup,
           "host_prior_ms_per_problem": host_ms, "rows": []}
    for B in (int(b) for b in args.batches.split(",")):
        row = measure(pkg, base_ics, host_ms, host_arrays, args.ns, args.nt, B, args.reps, args.warmup)
        out["rows"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
