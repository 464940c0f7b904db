"""Latency of the batched Gauss-Newton driver bound to the nonlinear elliptic tangent (gmrf_gn_create_elliptic) on elliptic512
(n = 262 144, 256 blocks of 1024), one process, one stream, at batch 8 and the largest batch that fits.

Per batch size, medians of --reps after --warmup:
  gn_iter_ms            time of one iteration of gmrf_gn_run: (run of --steps iterations - run of 1 iteration) / (--steps - 1),
                        rtol = 0 so that no problem stops early
  tangent_ms            one `tangent_batch` call on device tensors between two events on the handle's stream: the kernel plus the
                        call's closing stream synchronisation (an upper bound of the kernel's time)
  tangent_gbytes_per_s  the bytes the kernel must stream per row -- 7 values and f written, w read: 72 B (border rows hold fewer
                        values; nnz is counted exactly) -- over tangent_ms: a lower bound of the achieved rate
  problems_per_s        batch / the whole run of --steps iterations
The largest batch: the device memory one problem takes is measured on the batch-8 handle (free memory before and after its
set-up and first run), and --fill (default 0.8) of what is free is given to the batch, capped at --max-batch.  The batch repeats
4 distinct problems (workloads.elliptic_gauss_newton_batch, amp = 0, 0.5, 1, 2).  Prints one JSON line.

--order 2 --nx 101 --ny 103: the reference's default quadratic triangles on 100 x 102 elements -- a 201 x 205 lattice, n = 41 205,
41 blocks of 1005 at 5 rows per block, the closest mesh to the reference's N_el_xy = 100 that partitions.  The bytes per row are
then the row's values (nnz counted exactly), f and w.  With --order 2 every row also holds
  refactor_solve_ms     `refactor` + `solve_batch` alone on the same handle and the values of the start point, device tensors
  glue_ratio            gn_iter_ms / refactor_solve_ms (the project's bar for driver glue is 1.10)
  p1_tangent_*          the P1 kernel's `tangent_batch` at the same batch on --p1-n-xy (512) nodes per side, measured in the same
                        run in the same way: the comparison for tangent_gbytes_per_s"""
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


def _tangent_rate(tan, x, stream, reps, warmup):
    """median / min time of `tangent_batch(x)` between two events on the stream, the bytes it must stream and the rate"""
    import torch
    t = []
    with torch.cuda.stream(stream):
        for i in range(warmup + max(reps, 10)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            tan.tangent_batch(x)
            e1.record(stream)
            e1.synchronize()
            if i >= warmup:
                t.append(e0.elapsed_time(e1))
    nbytes = 8 * x.shape[0] * (tan.nnz + 2 * tan.n)
    return statistics.median(t), min(t), nbytes, nbytes / (statistics.median(t) * 1e-3) / 1e9


def measure(pkg, base, B, steps, reps, warmup, p1_n_xy=512):
    import numpy as np
    import torch
    order = base.get("order", 1)
    idx = np.arange(B) % base["x0"].shape[0]
    noise = base["noise"]
    free0 = torch.cuda.mem_get_info()[0]
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    tan = pkg.EllipticP1Tangent(base["nx"], base["ny"], stream=s, order=order)
    asm = pkg.PosteriorAssembler(base["Q"], tan.pattern, stream=s)
    F = pkg.TridiagonalCholeskyFactor(stream=s, batch=B)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()          # noqa: E731
    q = dev(base["q_values"])
    qx, xp, x0 = dev(base["Qx_prior"][idx]), dev(base["x_prior"][idx]), dev(base["x0"][idx])
    y = tan.load(dev(base["src_q"][idx]))
    jv, _ = tan.tangent_batch(x0)
    a = asm.precision_batch(q, jv, noise)
    F.factor(asm.pattern, base["n_blocks"], values=a.cpu().numpy())
    del a, jv
    gn = pkg.GaussNewtonBatch(F, asm, tan)
    run = lambda k: gn.run(q, qx, xp, x0, y=y, noise=noise, rtol=0.0, max_steps=k)      # noqa: E731
    x, st, _ = run(steps)
    assert int(st.min()) == steps, st
    torch.cuda.synchronize()
    used = free0 - torch.cuda.mem_get_info()[0]
    err = pkg.workloads.solution_errors(x[2 % B].cpu().numpy(), base["truth"][idx[2 % B]])
    r = {"batch": B, "steps": steps, "n": base["n"], "n_blocks": base["n_blocks"], "device_bytes_per_problem": used / B,
         "rel_err_vs_truth_amp1_after_steps": err["rel_err"]}
    t_full = _median_ms(lambda: run(steps), reps, warmup)
    t_one = _median_ms(lambda: run(1), reps, warmup)
    r["gn_run_ms"] = t_full
    r["gn_iter_ms"] = (t_full - t_one) / (steps - 1)
    r["problems_per_s"] = B / (t_full * 1e-3)
    # the tangent kernel alone, on the iterate the run left
    r["tangent_ms"], r["tangent_ms_min"], r["tangent_bytes"], r["tangent_gbytes_per_s"] = _tangent_rate(tan, x, stream, reps, warmup)
    r["tangent_share_of_iteration"] = 2 * r["tangent_ms"] / r["gn_iter_ms"]      # (two launches per iteration: at x and at the candidate)
    if order == 2:
        r["order"], r["nx"], r["ny"], r["block_size"] = 2, base["nx"], base["ny"], F.stats()["block_size"]
        jv, _ = tan.tangent_batch(x0)
        a = asm.precision_batch(q, jv, noise)
        rhs = y.reshape(B, 1, -1).contiguous()

        def refactor_solve():
            F.refactor(a)
            F.solve_batch(rhs)

        r["refactor_solve_ms"] = _median_ms(refactor_solve, reps, warmup)
        r["glue_ratio"] = r["gn_iter_ms"] / r["refactor_solve_ms"]
        del a, jv, rhs
        p1 = pkg.EllipticP1Tangent(p1_n_xy, p1_n_xy, stream=s)
        xs = torch.from_numpy(np.random.default_rng(0).standard_normal((B, p1.n))).cuda()
        r["p1_n_xy"] = p1_n_xy
        r["p1_tangent_ms"], r["p1_tangent_ms_min"], r["p1_tangent_bytes"], r["p1_tangent_gbytes_per_s"] = _tangent_rate(p1, xs, stream, reps, warmup)
        r["tangent_rate_over_p1"] = r["tangent_gbytes_per_s"] / r["p1_tangent_gbytes_per_s"]
        del p1, xs
    gn.close(); F.close()
    del gn, F, asm, tan, q, qx, xp, x0, y, x
    torch.cuda.empty_cache()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--n-xy", type=int, default=512)
    ap.add_argument("--order", type=int, default=1, choices=(1, 2))
    ap.add_argument("--nx", type=int, default=101, help="order 2: vertices in x")
    ap.add_argument("--ny", type=int, default=103, help="order 2: vertices in y; rows-per-block must divide 2 ny - 1")
    ap.add_argument("--rows-per-block", type=int, default=5, help="order 2: lattice rows per block (at least 4)")
    ap.add_argument("--p1-n-xy", type=int, default=512, help="order 2: the mesh of the P1 kernel measured beside it")
    ap.add_argument("--batches", default="8,max", help="comma list; `max`: the largest batch that fits (needs an earlier entry)")
    ap.add_argument("--fill", type=float, default=0.8)
    ap.add_argument("--max-batch", type=int, default=64)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    pkg = g.load_package()
    if args.order == 2:
        base = pkg.workloads.elliptic_gauss_newton_batch((args.nx, args.ny), 4, rows_per_block=args.rows_per_block, amps=(0.0, 0.5, 1.0, 2.0), order=2)
        name = f"elliptic_p2_{args.nx}x{args.ny}"
    else:
        base = pkg.workloads.elliptic_gauss_newton_batch(args.n_xy, 4, amps=(0.0, 0.5, 1.0, 2.0))
        name = f"elliptic{args.n_xy}"
    out = {"tool": "elliptic_gn_latency", "workload": name, "reps": args.reps, "warmup": args.warmup, "rows": []}
    for b in args.batches.split(","):
        if b == "max":
            per = out["rows"][-1]["device_bytes_per_problem"]
            B = max(1, min(args.max_batch, int(args.fill * torch.cuda.mem_get_info()[0] / per)))
        else:
            B = int(b)
        row = measure(pkg, base, B, args.steps, args.reps, args.warmup, args.p1_n_xy)
        out["rows"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
