"""Latency of the batched Darcy conditioning driver (gmrf_dc_run) on darcy256, one process, one stream, batch 8 / 32 / 64.

Per batch size, medians of --reps after --warmup, device time by events on the stream, the two alternating in the process:
  run_ms        `DarcyConditioningBatch.run` with k_samples = 1, var = "rbmc", k_var = 50 (device tensors in and out)
  composed_ms   the same work from the calls that exist without the driver: the recipe of bench.py's `full_loop` -- per
                problem `assemble`, `precision`, `rhs`; `refactor`, `solve_batch`, `sample_batch(1)`,
                `marginal_var("rbmc", 50, q_values=...)` on the batch -- under its four timers
  std_share_*   the "Std dev" part of either: the driver's run with var = "rbmc" minus its run with var = None
The batch repeats 8 coefficient fields (workloads.darcy_coefficient).  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(pkg, n_xy, B, reps, warmup):
    import numpy as np
    import torch
    W = pkg.workloads
    q_eps = 1e8
    Q0, _, N = W.darcy_conditioning(n_xy)
    n = n_xy * n_xy
    gq = np.linspace(0.0, 1.0, 241)
    GX, GY = np.meshgrid(gq, gq, indexing="ij")
    tabs = [W.darcy_coefficient(523802340 + p)(GX.ravel(), GY.ravel()).reshape(241, 241) for p in range(min(8, B))]
    st = torch.cuda.Stream()
    s = st.cuda_stream
    tables = torch.from_numpy(np.stack([tabs[p % len(tabs)] for p in range(B)])).cuda()
    d = pkg.DarcyP1Assembler(n_xy, n_xy, stream=s)
    asm = pkg.PosteriorAssembler(Q0, d.pattern, stream=s)
    qd = torch.from_numpy(Q0.data).cuda()
    zero = torch.zeros(n, dtype=torch.float64, device="cuda")
    nz = torch.empty((B, asm.nnz_out), dtype=torch.float64, device="cuda")
    rhs = torch.empty((B, 1, n), dtype=torch.float64, device="cuda")
    v_rb = torch.empty((B, n), dtype=torch.float64, device="cuda")
    F = pkg.TridiagonalCholeskyFactor(stream=s, batch=B)
    F.set_keep_l(False)
    Qc = None

    def composed(first=False):
        nonlocal Qc
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        ev[0].record(st)
        av, yv = [], []
        for p in range(B):                                   # "PDE Discretization"
            a, y = d.assemble(tables[p])
            av.append(a); yv.append(y)
        ev[1].record(st)
        for p in range(B):                                   # "Conditioning"
            nz[p] = asm.precision(qd, av[p], q_eps)
            rhs[p, 0] = asm.rhs(None, av[p], zero, yv[p], q_eps)
        if first:
            P = asm.pattern.copy()
            P.data = nz[0].cpu().numpy()
            F.factor(P, N, values=nz.cpu().numpy())
            Qc = pkg.CsrMatrix(P, stream=s)
        else:
            F.refactor(nz)
        mu = F.solve_batch(rhs)[:, 0, :]
        ev[2].record(st)
        F.sample_batch(1, mean=mu, seed=7, like=rhs)          # "Sampling"
        ev[3].record(st)
        F.marginal_var("rbmc", k=50, seed=9, Q=Qc, q_values=nz, out=v_rb)     # "Std dev"
        torch.sqrt_(v_rb)
        ev[4].record(st)
        ev[4].synchronize()
        return [ev[i].elapsed_time(ev[i + 1]) for i in range(4)]

    with torch.cuda.stream(st):
        composed(True)
        dc = pkg.DarcyConditioningBatch(F, asm, d)
        out = pkg.DarcyConditioningResult(torch.empty((B, n), dtype=torch.float64, device="cuda"), torch.empty((B, 1, n), dtype=torch.float64, device="cuda"),
                                          torch.empty((B, n), dtype=torch.float64, device="cuda"), torch.empty(B, dtype=torch.float64, device="cuda"))
        out_nv = pkg.DarcyConditioningResult(out.mean, out.samples, None, None)

        def run(var):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            dc.run(tables, qd, q_eps=q_eps, k_samples=1, var=var, k_var=50, sample_seed=7, var_seed=9, out=out if var else out_nv)
            e1.record(st)
            e1.synchronize()
            return e0.elapsed_time(e1)

        for _ in range(warmup):
            run("rbmc"); composed(); run(None)
        t_run, t_cmp, t_nv = [], [], []
        for _ in range(reps):
            t_run.append(run("rbmc")); t_cmp.append(composed()); t_nv.append(run(None))
    cmp_med = np.median(np.array(t_cmp), axis=0)
    run_ms, nv_ms, composed_ms = statistics.median(t_run), statistics.median(t_nv), float(cmp_med.sum())
    r = {"batch": B, "run_ms": run_ms, "composed_ms": composed_ms, "run_over_composed": run_ms / composed_ms,
         "run_problems_per_s": B / (run_ms * 1e-3), "composed_problems_per_s": B / (composed_ms * 1e-3),
         "composed_timers_ms": {k: float(v) for k, v in zip(("pde_discretization", "conditioning_incl_mean", "sampling_1", "std_rbmc50"), cmp_med)},
         "run_without_std_ms": nv_ms, "std_share_run": (run_ms - nv_ms) / run_ms, "std_share_composed": float(cmp_med[3]) / composed_ms,
         "persist_aborts": F.stats()["persist_aborts"]}
    dc.close(); F.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batches", default="8,32,64")
    ap.add_argument("--n", type=int, default=256)
    args = ap.parse_args()
    import __graft_entry__ as g
    pkg = g.load_package()
    out = {"tool": "darcy_batch_latency", "workload": f"darcy{args.n}", "reps": args.reps, "warmup": args.warmup, "rows": []}
    for B in (int(b) for b in args.batches.split(",")):
        row = measure(pkg, args.n, B, args.reps, args.warmup)
        out["rows"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
