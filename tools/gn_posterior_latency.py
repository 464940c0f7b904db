"""Latency of the posterior stage of the batched Gauss-Newton driver on burgers512x64, one process, one stream, batch 8 / 32:
everything `solve_problem` returns for the final iterates of a run -- k_samples samples, RBMC(k_var) standard deviations and
their norms, logdet, sqmahal, nll and the error metrics against z.

Per batch size, medians (and minima) of --reps after --warmup, each timed call ending in a synchronisation:
  stage_ms        `GaussNewtonBatch.posterior` (gmrf_gn_posterior): one call, device tensors in and out
  composed_ms     the same results from the public calls a tree without that stage has: `finalize`, `sample_batch`, the posterior
                  values again (`tangent_batch` + `precision_batch`: the batch variance call wants them), `marginal_var` of the
                  batch, sqrt and norm on the host, B x (`select_problem` + `logdet`), sqmahal in SciPy on the downloaded values,
                  nll on the host, `solution_errors_batch`
  device_only_ms  the device part of that composition alone: `finalize` + `sample_batch` + the values + `marginal_var` into a
                  device tensor; no download
  values_ms       `tangent_batch` + `precision_batch` alone (inside both figures above)
--mode stage / composed / both: `composed` runs on a tree that has no `posterior` (an A/B against another checkout's build: run
this file from that checkout).  The batch repeats 8 distinct problems.  Prints one JSON line."""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _times_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return {"median": statistics.median(t), "min": min(t), "max": max(t)}


def measure(pkg, base, args, B, modes):
    import numpy as np
    import scipy.sparse as sp
    import torch
    ns, nt = args.ns, args.nt
    idx = np.arange(B) % base["x0"].shape[0]
    w = {k: (np.ascontiguousarray(v[idx]) if isinstance(v, np.ndarray) and v.ndim == 2 else v) for k, v in base.items()}
    noise = w["noise"]
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    tan = pkg.BurgersP1Tangent(ns, nt, w["dt"], w["nu"], stream=s)
    asm = pkg.PosteriorAssembler(w["Q"], tan.pattern, stream=s)
    F = pkg.TridiagonalCholeskyFactor(stream=s, batch=B)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()          # noqa: E731
    q, qx, xp, x0 = dev(w["q_values"]), dev(w["Qx_prior"]), dev(w["x_prior"]), dev(w["x0"])
    jv, _ = tan.tangent_batch(x0)
    a0 = asm.precision_batch(q, jv, noise)
    F.factor(asm.pattern, nt, values=a0.cpu().numpy())
    gn = pkg.GaussNewtonBatch(F, asm, tan)
    xd, st, _ = gn.run(q, qx, xp, x0, noise=noise, rtol=0.0, max_steps=args.steps)
    assert int(st.min()) == args.steps, st
    n = asm.n
    x = xd.cpu().numpy()
    xs, t = np.arange(ns) / ns, np.arange(nt)[:, None]
    z = x + 1e-3 * (np.sin(2 * np.pi * xs)[None, :] * np.cos(0.3 * t)).ravel()[None, :]
    zd = dev(z)
    k, kv = args.k_samples, args.k_var
    r = {"batch": B, "k_samples": k, "k_var": kv, "gn_steps": args.steps}
    check = {}

    if "stage" in modes:
        def stage():
            return gn.posterior(z=zd, first=ns, k_samples=k, var="rbmc", k_var=kv)
        res = stage()
        check["stage"] = (res.logdet.cpu().numpy(), res.sqmahal.cpu().numpy(), res.std_norm.cpu().numpy(), res.errors.cpu().numpy())
        r["stage_ms"] = _times_ms(stage, args.reps, args.warmup)

    if "composed" in modes:
        P = asm.pattern.copy()
        P.data = a0[0].cpu().numpy().copy()
        Qc = pkg.CsrMatrix(P, stream=s)
        var_dev = torch.empty((B, n), dtype=torch.float64, device="cuda")
        indptr, indices = asm.pattern.indptr, asm.pattern.indices

        def values():
            j, _ = tan.tangent_batch(xd)
            return asm.precision_batch(q, j, noise)

        def device_only():
            Ff = gn.finalize()
            smp = Ff.sample_batch(k, mean=xd)
            vals = values()
            Ff.marginal_var("rbmc", k=kv, Q=Qc, q_values=vals, out=var_dev)
            return Ff, smp, vals

        def composed():
            Ff, smp, vals = device_only()
            std = np.sqrt(var_dev.cpu().numpy())
            nrm = np.linalg.norm(std, axis=1)
            ld = np.empty(B)
            for p in range(B):
                Ff.select_problem(p)
                ld[p] = Ff.logdet()
            Ff.select_problem(0)
            vh = vals.cpu().numpy()
            sq = np.empty(B)
            for p in range(B):
                d = z[p] - x[p]
                sq[p] = d @ (sp.csc_matrix((vh[p], indices, indptr), shape=(n, n)) @ d)
            nll = 0.5 * ((n * math.log(2.0 * math.pi) + sq) - ld)
            err = pkg.solution_errors_batch(xd, zd, first=ns)
            return smp, std, nrm, ld, sq, nll, err

        res = composed()
        check["composed"] = (res[3], res[4], res[2], res[6])
        r["composed_ms"] = _times_ms(composed, args.reps, args.warmup)

        def device_only_synced():
            device_only()
            torch.cuda.synchronize()

        def values_synced():
            values()
            torch.cuda.synchronize()

        r["device_only_ms"] = _times_ms(device_only_synced, args.reps, args.warmup)
        r["values_ms"] = _times_ms(values_synced, args.reps, args.warmup)

    if len(check) == 2:          # the two routes computed the same things
        (ld_a, sq_a, nr_a, er_a), (ld_b, sq_b, nr_b, er_b) = check["stage"], check["composed"]
        assert np.array_equal(ld_a, ld_b) and np.array_equal(er_a, er_b)
        assert np.allclose(sq_a, sq_b, rtol=1e-9, atol=0.0) and np.allclose(nr_a, nr_b, rtol=1e-12, atol=0.0)
        r["stage_over_composed"] = r["stage_ms"]["median"] / r["composed_ms"]["median"]
    gn.close(); F.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2, help="Gauss-Newton iterations of the run in front of the stage (not timed)")
    ap.add_argument("--batches", default="8,32")
    ap.add_argument("--ns", type=int, default=512)
    ap.add_argument("--nt", type=int, default=64)
    ap.add_argument("--k-samples", type=int, default=1)
    ap.add_argument("--k-var", type=int, default=50)
    ap.add_argument("--mode", choices=("stage", "composed", "both"), default="both")
    args = ap.parse_args()
    import __graft_entry__ as g
    pkg = g.load_package()
    modes = ("stage", "composed") if args.mode == "both" else (args.mode,)
    if "stage" in modes and not hasattr(pkg.GaussNewtonBatch, "posterior"):
        raise SystemExit("this tree has no GaussNewtonBatch.posterior: --mode composed")
    base = pkg.workloads.burgers_gauss_newton_batch(args.ns, args.nt, 8, seed=0)
    out = {"tool": "gn_posterior_latency", "workload": f"burgers{args.ns}x{args.nt}", "mode": args.mode, "reps": args.reps,
           "warmup": args.warmup, "rows": []}
    for B in (int(b) for b in args.batches.split(",")):
        row = measure(pkg, base, args, B, modes)
        out["rows"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
