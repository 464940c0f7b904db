"""Latency of the batched Gauss-Newton driver bound to the Burgers collocation tangent at the shape of
scripts/burgers/solve_burgers_gmrf-collocation.jl's defaults (workloads.burgers_collocation_batch): N_basis = 750 quadratic cells
on the periodic unit line (ns = 1500), N_collocation = 750 points, and nt = 101 slices -- the data set's own slice count is not
available here, 101 is this tool's choice -- so n = 151 500 in 101 blocks of 1500; one process, one stream, at batches 1 and 8.

Per batch a row with (--runs times each, every figure listed):
  gn_iter_ms            time of one iteration of gmrf_gn_run: (run of --steps iterations - run of 1 iteration) / (--steps - 1),
                        rtol = 0 so that no problem stops early
  refactor_solve_ms     `refactor` + `solve_batch` alone on the same handle with the values of the start point, device tensors
  glue_ratio            median gn_iter_ms / median refactor_solve_ms
  tangent_ms            one `tangent_batch` call on device tensors between two events on the handle's stream (the kernel plus the
                        call's closing stream synchronisation: an upper bound of the kernel's time), with tangent_bytes, the bytes
                        it must stream (the values and f written, w read), and the rate they give
  steps                 a run to the stop rule (rtol 1e-4, at most 30 steps); the batch repeats 3 initial conditions
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DISTINCT = 3


def _ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


class Loop:
    """Handle, assembler, tangent and driver at one batch on one stream."""

    def __init__(self, pkg, base, B):
        import numpy as np
        import torch
        self.pkg, self.base, self.B, self.noise = pkg, base, B, base["noise"]
        idx = np.arange(B) % base["x0"].shape[0]
        self.stream = torch.cuda.Stream()
        s = self.stream.cuda_stream
        self.tan = pkg.BurgersCollocationTangent(base["nc"], base["n_blocks"], base["dt"], base["nu"], base["points"],
                                                 length=base["length"], stream=s)
        self.asm = pkg.PosteriorAssembler(base["Q"], self.tan.pattern, stream=s)
        self.F = pkg.TridiagonalCholeskyFactor(stream=s, batch=B)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()          # noqa: E731
        self.q, self.qx = dev(base["q_values"][idx]), dev(base["Qx_prior"][idx])
        self.xp, self.x0 = dev(base["x_prior"][idx]), dev(base["x0"][idx])
        jv, _ = self.tan.tangent_batch(self.x0)
        self.a0 = self.asm.precision_batch(self.q, jv, self.noise)
        self.F.factor(self.asm.pattern, base["n_blocks"], values=self.a0.cpu().numpy())
        self.gn = pkg.GaussNewtonBatch(self.F, self.asm, self.tan)

    def run(self, k, rtol=0.0):
        return self.gn.run(self.q, self.qx, self.xp, self.x0, noise=self.noise, rtol=rtol, max_steps=k)

    def iter_ms(self, steps):
        return (_ms(lambda: self.run(steps)) - _ms(lambda: self.run(1))) / (steps - 1)

    def refactor_solve_ms(self):
        rhs = self.qx.reshape(self.B, 1, -1).contiguous()

        def go():
            self.F.refactor(self.a0)
            self.F.solve_batch(rhs)
        return _ms(go)

    def tangent_ms(self, reps=10, warmup=2):
        import torch
        t = []
        with torch.cuda.stream(self.stream):
            for i in range(warmup + reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(self.stream)
                self.tan.tangent_batch(self.x0)
                e1.record(self.stream)
                e1.synchronize()
                if i >= warmup:
                    t.append(e0.elapsed_time(e1))
        return statistics.median(t), min(t)

    def close(self):
        self.gn.close(); self.F.close()


def measure(pkg, base, B, steps, runs):
    import torch
    lp = Loop(pkg, base, B)
    row = {"batch": B, "n": base["n"], "n_blocks": base["n_blocks"], "block_size": lp.F.stats()["block_size"], "rows_of_J": lp.tan.rows,
           "steps_timed": steps, "gn_iter_ms": [], "refactor_solve_ms": []}
    lp.run(steps)                                  # warm-up
    lp.refactor_solve_ms()
    for _ in range(runs):
        row["gn_iter_ms"].append(lp.iter_ms(steps))
        row["refactor_solve_ms"].append(lp.refactor_solve_ms())
    row["glue_ratio"] = statistics.median(row["gn_iter_ms"]) / statistics.median(row["refactor_solve_ms"])
    row["tangent_ms"], row["tangent_ms_min"] = lp.tangent_ms()
    row["tangent_bytes"] = 8 * B * (lp.tan.nnz + lp.tan.rows + lp.tan.n)
    row["tangent_gbytes_per_s"] = row["tangent_bytes"] / (row["tangent_ms"] * 1e-3) / 1e9
    row["tangent_share_of_iteration"] = 2 * row["tangent_ms"] / statistics.median(row["gn_iter_ms"])
    _, st, hist = lp.run(30, 1e-4)
    row["steps"] = st.tolist()
    row["objective_first_last"] = [[float(hist[p, 0]), float(hist[p, st[p]])] for p in range(B)]
    lp.close()
    del lp
    torch.cuda.empty_cache()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nc", type=int, default=750)
    ap.add_argument("--npts", type=int, default=750)
    ap.add_argument("--nt", type=int, default=101)
    ap.add_argument("--nu", type=float, default=0.01)
    ap.add_argument("--T", type=float, default=1.0)
    ap.add_argument("--amp", type=float, default=0.5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--batches", default="1,8")
    args = ap.parse_args()
    import __graft_entry__ as g
    pkg = g.load_package()
    base = pkg.workloads.burgers_collocation_batch(args.nc, args.nt, args.npts, DISTINCT, args.nu, args.T, args.amp)
    out = {"tool": "burgers_colloc_latency", "workload": f"burgers_collocation_{args.nc}x{args.nt}x{args.npts}",
           "note": "N_basis and N_collocation are the script's defaults; the data set's own slice count is not available here, nt is this tool's choice",
           "nu": args.nu, "T": args.T, "dt": base["dt"], "amp": args.amp, "noise": base["noise"], "runs": args.runs, "rows": []}
    for b in args.batches.split(","):
        row = measure(pkg, base, int(b), args.steps, args.runs)
        out["rows"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
