"""Latency of the batched Burgers initial-condition stage (gmrf_bic_run) bound to the line prior (`BurgersLinePrior`), one process,
one stream: tools/burgers_ic_latency.py for any (order, bc, length).

Per batch size, medians of --reps after --warmup:
  ic_stage_ms           (a) `BurgersInitialConditionBatch.run` on device tensors: initial conditions -> bulk, prior values,
                        information vector -> refactor -> x_ic
  prior_ms              `BurgersLinePrior.values_batch` alone on device tensors (the three kernels and the call's synchronisation)
  refactor_solve_ms     (b) `refactor` + `solve_batch` alone on the same handle and the same values, device tensors
  glue_ratio            (a) / (b)
  host_route_ms_per_problem
                        (c) the route the stage replaces: `workloads.burgers_line_prior_from_bulk` and the assembly of Q_ic for ONE
                        problem on the host plus the upload of a batch's q_values, Qx_prior, x_prior, x0 divided by the batch; with
                        --host-solve also SuperLU's factorisation and solve for x_prior, as `workloads.burgers_chen24_batch` has it
  host_over_device      (c) / ((a) / batch)
The batch repeats 8 distinct initial conditions (a sum of two sines plus a bulk speed; on a dirichlet line zero at the ends).
Prints one JSON line."""
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


def measure(pkg, args, base_ics, host_ms, B):
    import numpy as np
    import torch
    ns, nt, fem_noise = base_ics.shape[1], args.nt, 1e12
    dt = 1.0 / (nt - 1)
    ics = np.ascontiguousarray(base_ics[np.arange(B) % base_ics.shape[0]])
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    prior = pkg.BurgersLinePrior(args.nc, nt, dt, args.nu, order=args.order, bc=args.bc, length=args.length, ic_noise=args.ic_noise, stream=s)
    tan = pkg.BurgersP1Tangent(ns, nt, dt, args.nu, stream=s, order=args.order, scheme=args.scheme, bc=args.bc, length=args.length)
    asm = pkg.PosteriorAssembler(prior.pattern, tan.pattern, stream=s)
    F = pkg.TridiagonalCholeskyFactor(stream=s, batch=B)
    d_ics = torch.from_numpy(ics).cuda()
    v = prior.values_batch(d_ics)
    x0 = v["bulk"][:, None].repeat(1, ns * nt).contiguous()
    x0[:, :ns] = d_ics
    jv, _ = tan.tangent_batch(x0)
    F.factor(asm.pattern, nt, values=asm.precision_batch(v["q_values"], jv, fem_noise).cpu().numpy())
    stage = pkg.BurgersInitialConditionBatch(F, asm, prior)
    r = {"batch": B}
    r["ic_stage_ms"] = _median_ms(lambda: stage.run(d_ics), args.reps, args.warmup)
    r["prior_ms"] = _median_ms(lambda: prior.values_batch(d_ics), args.reps, args.warmup)
    # (b): Q_ic's values in the assembler's order (J = 0, noise 0) and the same right-hand side, nothing else
    a = asm.precision_batch(v["q_values"], torch.zeros_like(jv), 0.0)
    rhs = v["Qx_prior"].reshape(B, 1, -1).contiguous()

    def refactor_solve():
        F.refactor(a)
        F.solve_batch(rhs)

    r["refactor_solve_ms"] = _median_ms(refactor_solve, args.reps, args.warmup)
    r["glue_ratio"] = r["ic_stage_ms"] / r["refactor_solve_ms"]
    # (c): the upload of a batch of host priors
    up = [np.zeros((B, prior.nnz)), np.zeros((B, prior.n)), np.zeros((B, prior.n)), np.zeros((B, prior.n))]

    def upload():
        for arr in up:
            torch.from_numpy(arr).cuda()
        torch.cuda.synchronize()

    r["upload_ms_per_problem"] = _median_ms(upload, args.reps, args.warmup) / B
    r["host_route_ms_per_problem"] = host_ms + r["upload_ms_per_problem"]
    r["device_ms_per_problem"] = r["ic_stage_ms"] / B
    r["host_over_device"] = r["host_route_ms_per_problem"] / r["device_ms_per_problem"]
    stage.close(); F.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--nc", type=int, default=512)
    ap.add_argument("--nt", type=int, default=64)
    ap.add_argument("--order", type=int, default=2)
    ap.add_argument("--bc", default="periodic")
    ap.add_argument("--length", type=float, default=1.0)
    ap.add_argument("--scheme", default="euler")
    ap.add_argument("--nu", type=float, default=0.01 / 3.141592653589793)
    ap.add_argument("--ic-noise", type=float, default=1e8)
    ap.add_argument("--host-solve", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import scipy.sparse.linalg as spla
    import __graft_entry__ as g
    pkg = g.load_package()
    W = pkg.workloads
    ns = args.order * args.nc + (1 if args.bc == "dirichlet" else 0)
    base_ics = W.burgers_initial_conditions(ns, 8) + 0.1 * np.arange(8)[:, None]          # (a bulk speed per problem)
    if args.bc == "dirichlet":
        base_ics[:, 0] = 0.0
        base_ics[:, -1] = 0.0
    obs = W.burgers_line_ic_observed(ns, args.order, args.bc)
    dt = 1.0 / (args.nt - 1)
    host = {}

    def host_prior():
        ic = base_ics[1]
        Qp, Aic, rhs = W.burgers_line_prior_from_bulk(args.nc, args.nt, dt, args.nu, float(ic[obs].mean()), ic, args.order, args.bc,
                                                      args.length, args.ic_noise)
        Q = (Qp + args.ic_noise * (Aic.T @ Aic)).tocsc()
        Q = ((Q + Q.T) * 0.5).tocsc()
        Q.sort_indices()
        host["Q"], host["rhs"] = Q, rhs

    host_prior_ms = _median_ms(host_prior, args.reps, args.warmup)
    host_solve_ms = _median_ms(lambda: spla.splu(host["Q"]).solve(host["rhs"]), args.reps, args.warmup) if args.host_solve else 0.0
    out = {"tool": "burgers_line_ic_latency", "workload": f"burgers_line order {args.order} {args.bc} {args.nc} cells x {args.nt} slices",
           "ns": ns, "n": ns * args.nt, "length": args.length, "nu": args.nu, "ic_noise": args.ic_noise, "scheme": args.scheme,
           "reps": args.reps, "warmup": args.warmup, "host_prior_ms_per_problem": host_prior_ms, "host_splu_solve_ms_per_problem": host_solve_ms,
           "rows": []}
    for B in (int(b) for b in args.batches.split(",")):
        row = measure(pkg, args, base_ics, host_prior_ms + host_solve_ms, B)
        out["rows"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
