"""Latency of the batched Gauss-Newton driver (gmrf_gn_run) on burgers512x64, one process, one stream, batch 8 / 32 / 64.

Per batch size, medians of --reps after --warmup:
  gn_iter_ms            time of one iteration of gmrf_gn_run: (run of --steps iterations - run of 1 iteration) / (--steps - 1),
                        rtol = 0 so that no problem stops early
  refactor_solve_ms     `refactor` + `solve_batch` alone on the same handle, device tensors
  glue_ratio            gn_iter_ms / refactor_solve_ms
  batched_problems_per_s / sequential_problems_per_s
                        the whole run of --steps iterations for the batch, beside the same problems one after the other
                        through the one-problem `gn_step` loop (a batch-1 handle, the same iteration count)
The batch repeats 8 distinct problems (initial conditions of workloads.burgers_gauss_newton_batch).  Prints one JSON line."""
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


def measure(pkg, base, ns, nt, B, steps, reps, warmup):
    import numpy as np
    import torch
    idx = np.arange(B) % base["x0"].shape[0]
    w = {k: (np.ascontiguousarray(v[idx]) if isinstance(v, np.ndarray) and v.ndim == 2 else v) for k, v in base.items()}
    noise = w["noise"]
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    tan = pkg.BurgersP1Tangent(ns, nt, w["dt"], w["nu"], stream=s)
    asm = pkg.PosteriorAssembler(w["Q"], tan.pattern, stream=s)
    F = pkg.TridiagonalCholeskyFactor(stream=s, batch=B)
    dev = lambda a: torch.from_numpy(a).cuda()          # noqa: E731
    q, qx, xp, x0 = dev(w["q_values"]), dev(w["Qx_prior"]), dev(w["x_prior"]), dev(w["x0"])
    jv, _ = tan.tangent_batch(x0)
    a = asm.precision_batch(q, jv, noise)
    F.factor(asm.pattern, nt, values=a.cpu().numpy())
    gn = pkg.GaussNewtonBatch(F, asm, tan)
    run = lambda k: gn.run(q, qx, xp, x0, noise=noise, rtol=0.0, max_steps=k)      # noqa: E731
    _, st, _ = run(steps)
    assert int(st.min()) == steps, st
    r = {"batch": B, "steps": steps}
    t_full = _median_ms(lambda: run(steps), reps, warmup)
    t_one = _median_ms(lambda: run(1), reps, warmup)
    r["gn_run_ms"] = t_full
    r["gn_iter_ms"] = (t_full - t_one) / (steps - 1)
    rhs = qx.reshape(B, 1, -1).contiguous()

    def refactor_solve():
        F.refactor(a)
        F.solve_batch(rhs)

    r["refactor_solve_ms"] = _median_ms(refactor_solve, reps, warmup)
    r["glue_ratio"] = r["gn_iter_ms"] / r["refactor_solve_ms"]
    r["batched_problems_per_s"] = B / (t_full * 1e-3)
    # the same problems one after the other: the one-problem device loop (a batch-1 handle on its own stream)
    b1 = pkg.BurgersP1Tangent(ns, nt, w["dt"], w["nu"])
    asm1 = pkg.PosteriorAssembler(w["Q"], b1.pattern)
    P = asm1.pattern.copy()
    P.data = a[0].cpu().numpy()
    F1 = pkg.tridiagonal_cholesky(P, nt)

    def sequential(count):
        for p in range(count):
            x = x0[p].clone()
            for _ in range(steps):
                j1, f1 = b1.tangent(x)
                x = pkg.gn_step(F1, asm1, q[p], qx[p], j1, x, -f1, noise)
        torch.cuda.synchronize()

    sequential(1)
    t0 = time.perf_counter()
    sequential(B)
    t_seq = time.perf_counter() - t0
    r["sequential_problems_per_s"] = B / t_seq
    r["batched_over_sequential"] = r["batched_problems_per_s"] / r["sequential_problems_per_s"]
    gn.close(); F.close(); F1.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--batches", default="8,32,64")
    ap.add_argument("--ns", type=int, default=512)
    ap.add_argument("--nt", type=int, default=64)
    args = ap.parse_args()
    import __graft_entry__ as g
    pkg = g.load_package()
    base = pkg.workloads.burgers_gauss_newton_batch(args.ns, args.nt, 8, seed=0)
    out = {"tool": "gn_batch_latency", "workload": f"burgers{args.ns}x{args.nt}", "reps": args.reps, "warmup": args.warmup, "rows": []}
    for B in (int(b) for b in args.batches.split(",")):
        row = measure(pkg, base, args.ns, args.nt, B, args.steps, args.reps, args.warmup)
        out["rows"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
