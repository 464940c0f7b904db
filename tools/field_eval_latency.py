"""Latency of the last line of the data-set loops -- fields at the data grid's points and their error metrics -- on the two shapes the
loops have, one stream, device tensors:
  darcy    quadratic triangles nx = ny = 129 (lattice 257^2, ns = 66 049), the 241 x 241 data grid, batch 8 / 32 / 64
  burgers  512 quadratic periodic cells x 64 slices (ns = 1024 per slice), 1024 points, the first slice left out, batch 8 / 32
Three legs per shape and batch, medians of --reps runs after --warmup, each timed call ending synchronised:
  a_fused_ms   `FieldEvaluator.errors` without pred (gmrf_eval_errors_batch): one pass, nothing of size batch nt npts written
  b_two_ms     `FieldEvaluator.apply`, then `solution_errors_batch` on its result
  c_host_ms    the route the evaluator replaces: the fields to the host, SciPy `E @ field`, NumPy metrics (E is built once, outside)
and per leg a / b the streamed bytes rows (ns + npts) 8 + table per second beside the 8 TB/s HBM peak, and c / a.
Every (shape, batch) runs in a child process of its own under --step-timeout; after a child that fails or runs out of time
nothing more is started.  Writes one JSON file (--out)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12
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


def child(shape, B, reps, warmup):
    import numpy as np
    import torch
    import __graft_entry__ as g
    pkg = g.load_package()
    stream = torch.cuda.Stream()
    rng = np.random.default_rng(0)
    if shape == "darcy":
        nx, nt, first_slice = 129, 1, 0
        grid = np.linspace(0.0, 1.0, 241)
        ev = pkg.FieldEvaluator.triangles(nx, nx, pkg.workloads.darcy_pred_coords(grid, grid), order=2, stream=stream.cuda_stream)
        lat = np.linspace(0.0, 1.0, 2 * nx - 1)
        base = (np.sin(np.pi * lat)[None, :] * np.sin(2 * np.pi * lat)[:, None]).ravel()
    else:
        nc, nt, first_slice = 512, 64, 1
        ev = pkg.FieldEvaluator.line(nc, pkg.workloads.burgers_pred_coords(np.arange(1024) / 1024.0), order=2, stream=stream.cuda_stream)
        base = (np.sin(2 * np.pi * np.arange(ev.ns) / ev.ns)[None, :] * np.cos(0.3 * np.arange(nt))[:, None]).ravel()
    fields = base[None, :] * (1.0 + 0.1 * rng.standard_normal((B, 1))) + 1e-3 * rng.standard_normal((B, nt * ev.ns))
    E = ev.matrix()
    rows, first = B * nt, first_slice * ev.npts
    truth = (E @ fields.reshape(rows, ev.ns).T).T.reshape(B, nt * ev.npts) + 1e-3 * rng.standard_normal((B, nt * ev.npts))
    fd, td = torch.from_numpy(fields).cuda(), torch.from_numpy(truth).cuda()
    torch.cuda.synchronize()

    def a():
        return ev.errors(fd, td, nt=nt, first_slice=first_slice)

    def b():
        return pkg.solution_errors_batch(ev.apply(fd.view(rows, ev.ns)).view(B, nt * ev.npts), td, first=first)

    def c():
        f = fd.cpu().numpy()
        d = ((E @ f.reshape(rows, ev.ns).T).T.reshape(B, nt * ev.npts) - truth)[:, first:]
        s = truth[:, first:]
        return np.stack([np.linalg.norm(d, axis=1) / np.linalg.norm(s, axis=1), np.sqrt(np.mean(d * d, axis=1)), np.max(np.abs(d), axis=1)],
                        axis=1)

    ra, rb, rc = a(), b(), c()
    assert np.array_equal(ra, rb), "the fused call and the two calls must give the same bits"
    assert np.allclose(ra, rc, rtol=1e-9, atol=0.0), (ra, rc)
    streamed = rows * (ev.ns + ev.npts) * 8 + ev.npts * ev.width * 12
    r = {"shape": shape, "batch": B, "ns": ev.ns, "npts": ev.npts, "nt": nt, "first_slice": first_slice, "width": ev.width,
         "streamed_bytes": streamed, "a_fused_ms": _times_ms(a, reps, warmup), "b_two_ms": _times_ms(b, reps, warmup),
         "c_host_ms": _times_ms(c, reps, warmup)}
    for leg in ("a_fused_ms", "b_two_ms"):
        rate = streamed / (r[leg]["median"] * 1e-3)
        r[leg]["bytes_per_s"], r[leg]["of_hbm_peak"] = rate, rate / HBM_PEAK
    r["c_over_a"] = r["c_host_ms"]["median"] / r["a_fused_ms"]["median"]
    r["a_over_b"] = r["a_fused_ms"]["median"] / r["b_two_ms"]["median"]
    ev.close()
    print(json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--step-timeout", type=float, default=120.0, help="seconds a (shape, batch) child may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r26_field_eval_latency.json"))
    ap.add_argument("--child", nargs=2, metavar=("SHAPE", "BATCH"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], int(args.child[1]), args.reps, args.warmup)
    out = {"tool": "field_eval_latency", "reps": args.reps, "warmup": args.warmup, "hbm_peak_bytes_per_s": HBM_PEAK, "rows": []}
    steps = [(s, B) for s, batches in SHAPES.items() for B in batches]
    for shape, B in steps:
        cmd = [sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--warmup", str(args.warmup), "--child", shape, str(B)]
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
        print(json.dumps(row), file=sys.stderr, flush=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"tool": out["tool"], "rows": len(out["rows"]), "out": args.out, "stopped": "stopped_at" in out}), flush=True)
    return 1 if "stopped_at" in out else 0


if __name__ == "__main__":
    sys.exit(main())
