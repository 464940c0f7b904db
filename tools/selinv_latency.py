"""Latency of the selected inverse on the pattern of Q (gmrf_bt_selinv) beside the exact marginal variances on the same factor.

darcy256, one problem and a batch of 64 (the pattern's values scaled per problem): selected_inverse, trace_inv
with m = 4 and marginal_var("exact"), median of --reps after --warmup, the pattern plan warm (built by the first call), outputs
in device tensors (`*_host_out_ms`: the same into NumPy arrays).  burgers512x64 and elliptic512, one problem: selected_inverse
and marginal_var("exact").  Prints one JSON line."""
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
    host = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        host.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(host)


def measure(pkg, w, batch, reps, warmup, trace=False):
    import numpy as np
    import scipy.sparse as sp
    import torch
    Q = sp.csc_matrix(w.Q)
    Q.sort_indices()
    S = pkg.CsrMatrix(Q)
    F = pkg.TridiagonalCholeskyFactor(batch=batch)
    F.factor(Q, w.n_blocks, values=None if batch == 1 else np.stack([Q.data * (1.0 + 0.001 * p) for p in range(batch)]))
    shape = (S.nnz,) if batch == 1 else (batch, S.nnz)
    out = np.empty(shape)
    r = {"batch": batch, "nnz": S.nnz}
    # device outputs (what the products cost), then host outputs (plus the copy to pageable memory)
    v_dev = torch.empty((w.n,) if batch == 1 else (batch, w.n), dtype=torch.float64, device="cuda")
    s_dev = torch.empty(shape, dtype=torch.float64, device="cuda")
    r["var_exact_ms"] = _median_ms(lambda: F.marginal_var("exact", out=v_dev), reps, warmup)
    r["selinv_ms"] = _median_ms(lambda: F.selected_inverse(S, out=s_dev), reps, warmup)
    if trace:
        dv = np.random.default_rng(1).standard_normal((4, S.nnz) if batch == 1 else (batch, 4, S.nnz))
        dv_dev = torch.from_numpy(dv).cuda()
        r["trace_inv_m4_ms"] = _median_ms(lambda: F.trace_inv(S, dv_dev), reps, warmup)
    r["selinv_over_var_exact"] = r["selinv_ms"] / r["var_exact_ms"]
    r["var_exact_host_out_ms"] = _median_ms(lambda: F.marginal_var("exact"), reps, warmup)
    r["selinv_host_out_ms"] = _median_ms(lambda: F.selected_inverse(S, out=out), reps, warmup)
    F.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--cases", default="darcy256,burgers512x64,elliptic512")
    args = ap.parse_args()
    import __graft_entry__ as g
    pkg = g.load_package()
    out = {"tool": "selinv_latency", "reps": args.reps, "warmup": args.warmup, "cases": {}}
    for name in args.cases.split(","):
        w = pkg.workloads.make(name)
        c = {"n": w.n, "n_blocks": w.n_blocks, "block_size": w.n // w.n_blocks}
        c["one"] = measure(pkg, w, 1, args.reps, args.warmup, trace=(name == "darcy256"))
        if name == "darcy256" and args.batch > 1:
            c[f"batch{args.batch}"] = measure(pkg, w, args.batch, max(3, args.reps // 3), 1, trace=True)
        out["cases"][name] = c
        print(json.dumps({name: c}), file=sys.stderr, flush=True)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
