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
4 distinct problems (workloads.elliptic_gauss_newton_batch, amp = 0, 0.5, 1, 2).  Prints one JSON line."""
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


def measure(pkg, base, B, steps, reps, warmup):
    import numpy as np
    import torch
    idx = np.arange(B) % base["x0"].shape[0]
    noise = base["noise"]
    free0 = torch.cuda.mem_get_info()[0]
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    tan = pkg.EllipticP1Tangent(base["nx"], base["ny"], stream=s)
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
    r["tangent_ms"] = statistics.median(t)
    r["tangent_ms_min"] = min(t)
    r["tangent_bytes"] = 8 * B * (tan.nnz + 2 * tan.n)
    r["tangent_gbytes_per_s"] = r["tangent_bytes"] / (r["tangent_ms"] * 1e-3) / 1e9
    r["tangent_share_of_iteration"] = 2 * r["tangent_ms"] / r["gn_iter_ms"]      # (two launches per iteration: at x and at the candidate)
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
    ap.add_argument("--batches", default="8,max", help="comma list; `max`: the largest batch that fits (needs an earlier entry)")
    ap.add_argument("--fill", type=float, default=0.8)
    ap.add_argument("--max-batch", type=int, default=64)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    pkg = g.load_package()
    base = pkg.workloads.elliptic_gauss_newton_batch(args.n_xy, 4, amps=(0.0, 0.5, 1.0, 2.0))
    out = {"tool": "elliptic_gn_latency", "workload": f"elliptic{args.n_xy}", "reps": args.reps, "warmup": args.warmup, "rows": []}
    for b in args.batches.split(","):
        if b == "max":
            per = out["rows"][-1]["device_bytes_per_problem"]
            B = max(1, min(args.max_batch, int(args.fill * torch.cuda.mem_get_info()[0] / per)))
        else:
            B = int(b)
        row = measure(pkg, base, B, args.steps, args.reps, args.warmup)
        out["rows"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
