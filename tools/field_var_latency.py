"""Latency of the pointwise predictive variance and of the calibration at the data grid's points on the two shapes the data-set loops
have, one stream, device tensors:
  darcy    workloads.make("darcy256"): P1 triangles nx = ny = 256 (n = 65 536, 64 blocks of 1024), the 241 x 241 data grid,
           batch 8 / 32 / 64
  burgers  512 quadratic periodic cells x 64 slices (workloads.burgers_line_prior_from_bulk with the initial condition observed:
           n = 65 536, 64 blocks of 1024), 1024 points, the first slice left out of the sums, batch 8 / 32
The problems of a batch are the workload's matrix with its diagonal scaled by 1 + 0.05 p.  Five legs per shape and batch, medians of
--reps runs after --warmup, each timed call ending synchronised:
  var_ms          `FieldEvaluator.variance` into a device tensor (gmrf_eval_var_batch)
  calibration_ms  `FieldEvaluator.calibration` of device fields against a device truth (gmrf_eval_calibration_batch)
  selinv_ms       `selected_inverse` on the same pattern `pair_pattern(nt)` alone, into a device tensor (gmrf_bt_selinv)
  marginal_ms     `marginal_var("exact")` into a device tensor: diag(Sigma) on the dofs
  host_ms         the same result from the calls that exist without the evaluator's: `selected_inverse` on Q's pattern to the host,
                  SciPy (E Sigma) o E per problem, NumPy metrics (E is built once, outside)
and the ratios host / calibration, var / selinv, var / marginal.  Every (shape, batch) runs in a child process of its own under
--step-timeout; after a child that fails or runs out of time nothing more is started.  --small: reduced shapes for a quick check.
Writes one JSON file (--out)."""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"darcy": (8, 32, 64), "burgers": (8, 32)}


def _times_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return {"median": statistics.median(t), "min": min(t), "max": max(t)}


def build_case(pkg, shape, small=False):
    """(Q csc sorted, n_blocks, nt, first_slice, evaluator arguments) of a shape."""
    import numpy as np
    import scipy.sparse as sp
    if shape == "darcy":
        w = pkg.workloads.make("darcy32" if small else "darcy256")
        nx = int(round(math.sqrt(w.n)))
        grid = np.linspace(0.0, 1.0, 31 if small else 241)
        return w.Q, w.n_blocks, 1, 0, ("triangles", (nx, nx, pkg.workloads.darcy_pred_coords(grid, grid)), {"order": 1})
    nc, nt = (16, 4) if small else (512, 64)
    ns = 2 * nc
    ic = np.sin(2 * np.pi * np.arange(ns) / ns) + 0.5 * np.sin(4 * np.pi * np.arange(ns) / ns + 0.3)
    Qp, Aic, _ = pkg.workloads.burgers_line_prior_from_bulk(nc, nt, 1.0 / (nt - 1), 0.01 / math.pi, float(ic.mean()), ic, order=2,
                                                            bc="periodic")
    Q = (Qp + 1e8 * (Aic.T @ Aic)).tocsc()
    Q = ((Q + Q.T) * 0.5).tocsc()
    Q.sort_indices()
    pts = pkg.workloads.burgers_pred_coords(np.arange(2 * ns if small else 1024) / float(2 * ns if small else 1024))
    return Q, nt, nt, 1, ("line", (nc, pts), {"order": 2, "bc": "periodic"})


def host_calibration(E, Q, vals, fields, truth, first, zcrit):
    """The calibration from Sigma on Q's pattern (vals (B, nnz) in Q's CSR order) on the host: SciPy and NumPy."""
    import numpy as np
    import scipy.sparse as sp
    out, var = [], []
    for p in range(vals.shape[0]):
        Sig = sp.csr_matrix((vals[p], Q.indices, Q.indptr), shape=Q.shape)
        v = np.asarray((E @ Sig).multiply(E).sum(axis=1)).ravel()
        z = ((E @ fields[p]) - truth[p])[first:] / np.sqrt(v[first:])
        out.append([np.mean(z * z), np.mean(np.abs(z) <= zcrit), np.mean(-0.5 * (np.log(2 * np.pi * v[first:]) + z * z)), v[first:].min()])
        var.append(v)
    return np.array(out), np.stack(var)


def child(shape, B, reps, warmup, small):
    import numpy as np
    import scipy.sparse as sp
    import torch
    import __graft_entry__ as g
    pkg = g.load_package()
    stream = torch.cuda.Stream()
    rng = np.random.default_rng(0)
    zcrit = 1.96
    Q, n_blocks, nt, first_slice, (kind, ev_args, ev_kw) = build_case(pkg, shape, small)
    ev = getattr(pkg.FieldEvaluator, kind)(*ev_args, stream=stream.cuda_stream, **ev_kw)
    n, first = Q.shape[0], first_slice * ev.npts
    diag = sp.diags(Q.diagonal()).tocsc()
    mats = []
    for p in range(B):
        M = (Q + 0.05 * p * diag).tocsc()
        M.sort_indices()
        assert np.array_equal(M.indptr, Q.indptr) and np.array_equal(M.indices, Q.indices)
        mats.append(M.data)
    F = pkg.TridiagonalCholeskyFactor(batch=B, stream=stream.cuda_stream)
    F.factor(Q, n_blocks, values=np.stack(mats))
    del mats
    K = ev.pair_pattern(nt)
    Kd = pkg.CsrMatrix(K, stream=stream.cuda_stream)
    Qcsr = sp.csr_matrix(Q)
    Qcsr.sort_indices()
    Qd = pkg.CsrMatrix(Qcsr, stream=stream.cuda_stream)
    E = ev.matrix(nt=nt)
    var_d = torch.empty((B, nt, ev.npts), dtype=torch.float64, device="cuda")
    sel_d = torch.empty((K.nnz,) if B == 1 else (B, K.nnz), dtype=torch.float64, device="cuda")
    mv_d = torch.empty((n,) if B == 1 else (B, n), dtype=torch.float64, device="cuda")
    fields = rng.standard_normal((B, n))
    fd = torch.from_numpy(fields).cuda()
    var0 = ev.variance(F, nt).reshape(B, nt * ev.npts)
    truth = ev.apply(fields.reshape(B * nt, ev.ns)).reshape(B, nt * ev.npts) + np.sqrt(var0) * rng.standard_normal((B, nt * ev.npts))
    td = torch.from_numpy(truth).cuda()
    torch.cuda.synchronize()

    def leg_var():
        return ev.variance(F, nt, out=var_d)

    def leg_cal():
        return ev.calibration(F, fd, td, nt=nt, first_slice=first_slice, zcrit=zcrit)

    def leg_sel():
        return F.selected_inverse(Kd, out=sel_d)

    def leg_marginal():
        return F.marginal_var("exact", out=mv_d)

    def leg_host():
        vals = F.selected_inverse(Qd, out=np.empty((Qcsr.nnz,) if B == 1 else (B, Qcsr.nnz))).reshape(B, Qcsr.nnz)
        return host_calibration(E, Qcsr, vals, fields, truth, first, zcrit)

    got = leg_cal()
    want, var_h = leg_host()
    # (both come from the same factor: they differ by the order of their sums; recorded below, refused only when grossly apart)
    assert np.allclose(var0, var_h, rtol=1e-3, atol=0.0) and np.allclose(got, want, rtol=1e-2, atol=1e-2), (got, want)
    r = {"shape": shape, "batch": B, "n": n, "n_blocks": n_blocks, "ns": ev.ns, "npts": ev.npts, "nt": nt, "first_slice": first_slice,
         "width": ev.width, "nnz_pair_pattern": int(K.nnz), "nnz_q": int(Qcsr.nnz), "calibration": got.tolist(),
         "calibration_host": want.tolist(), "max_rel_var_device_vs_host": float(np.max(np.abs(var0 - var_h) / var_h)),
         "var_ms": _times_ms(leg_var, reps, warmup), "calibration_ms": _times_ms(leg_cal, reps, warmup),
         "selinv_ms": _times_ms(leg_sel, reps, warmup), "marginal_ms": _times_ms(leg_marginal, reps, warmup),
         "host_ms": _times_ms(leg_host, reps, warmup)}
    r["host_over_calibration"] = r["host_ms"]["median"] / r["calibration_ms"]["median"]
    r["var_over_selinv"] = r["var_ms"]["median"] / r["selinv_ms"]["median"]
    r["var_over_marginal"] = r["var_ms"]["median"] / r["marginal_ms"]["median"]
    r["persist_aborts"] = int(F.stats().get("persist_aborts", 0))
    ev.close()
    F.close()
    print(json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--step-timeout", type=float, default=240.0, help="seconds a (shape, batch) child may take")
    ap.add_argument("--small", action="store_true", help="reduced shapes (darcy32 and a 31 x 31 grid; 16 cells x 4 slices)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r28_field_var_latency.json"))
    ap.add_argument("--child", nargs=2, metavar=("SHAPE", "BATCH"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], int(args.child[1]), args.reps, args.warmup, args.small)
    out = {"tool": "field_var_latency", "reps": args.reps, "warmup": args.warmup, "small": args.small, "rows": []}
    steps = [(s, B) for s, batches in SHAPES.items() for B in batches]
    for shape, B in steps:
        cmd = [sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--warmup", str(args.warmup), "--child", shape, str(B)]
        if args.small:
            cmd.append("--small")
        try:
            p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=args.step_timeout)
            rc, tail = p.returncode, (p.stdout + p.stderr)[-2000:]
        except subprocess.TimeoutExpired:
            rc, tail = 124, "timed out"
        if rc != 0:                     # nothing more is started on the device after a step that failed
            out["stopped_at"] = {"shape": shape, "batch": B, "rc": rc, "tail": tail}
            break
        row = json.loads(p.stdout.strip().splitlines()[-1])
        out["rows"].append(row)
        print(json.dumps({k: v for k, v in row.items() if k != "calibration"}), file=sys.stderr, flush=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"tool": out["tool"], "rows": len(out["rows"]), "out": args.out, "stopped": "stopped_at" in out}), flush=True)
    return 1 if "stopped_at" in out else 0


if __name__ == "__main__":
    sys.exit(main())
