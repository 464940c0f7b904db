"""Latency and accuracy of the batched Gauss-Newton driver bound to the Burgers line tangent on the benchmark of
_research/burgers_chen24.jl (workloads.burgers_chen24_batch): nc = 1000 quadratic cells on [-1, 1] with Dirichlet ends (ns = 2001),
nt = 51 slices (dt = 0.02), nu = 0.001 -- n = 102 051 in 51 blocks of 2001 --, one process, one stream, at batches 1 and 8.

Per batch a row with, for implicit Euler and Crank-Nicolson measured ALTERNATELY (--runs times each, every figure listed):
  gn_iter_ms            time of one iteration of gmrf_gn_run: (run of --steps iterations - run of 1 iteration) / (--steps - 1),
                        rtol = 0 so that no problem stops early
  refactor_solve_ms     `refactor` + `solve_batch` alone on the same handle with the values of the start point, device tensors
  glue_ratio            median gn_iter_ms / median refactor_solve_ms
  tangent_ms            one `tangent_batch` call on device tensors between two events on the handle's stream (the kernel plus the
                        call's closing stream synchronisation: an upper bound of the kernel's time), with tangent_bytes, the bytes
                        it must stream (the values and f written, w read), and the rate they give
  steps, rel_err, max_err   a run to the stop rule (rtol 1e-4, at most 30 steps) against Cole-Hopf at T = 1 on the last slice
                        (solution_errors_batch); the batch repeats the amplitudes 1.0, 0.5, 1.3
and, once at batch 1 with Crank-Nicolson, the reference's fem_noise = 1e18: the steps and errors if it factors, else the failing
block and the largest power of ten below it that factors.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

AMPS = (1.0, 0.5, 1.3)


def _ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


class Loop:
    """Handle, assembler, tangent and driver of one scheme at one batch on one stream."""

    def __init__(self, pkg, base, scheme, B, noise=None):
        import numpy as np
        import torch
        self.pkg, self.base, self.B, self.scheme = pkg, base, B, scheme
        self.noise = base["noise"] if noise is None else noise
        idx = np.arange(B) % base["x0"].shape[0]
        self.stream = torch.cuda.Stream()
        s = self.stream.cuda_stream
        self.tan = pkg.BurgersP1Tangent(base["ns"], base["n_blocks"], base["dt"], base["nu"], stream=s, order=base["order"],
                                        scheme=scheme, bc="dirichlet", length=base["length"])
        self.asm = pkg.PosteriorAssembler(base["Q"], self.tan.pattern, stream=s)
        self.F = pkg.TridiagonalCholeskyFactor(stream=s, batch=B)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()          # noqa: E731
        self.q = dev(base["q_values"][0])
        self.qx, self.xp, self.x0 = dev(base["Qx_prior"][idx]), dev(base["x_prior"][idx]), dev(base["x0"][idx])
        soln = np.zeros((B, base["n"]))
        soln[:, -base["ns"]:] = base["truth"][idx]
        self.soln = dev(soln)
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

    def to_stop_rule(self, rtol=1e-4, max_steps=30):
        x, steps, _ = self.run(max_steps, rtol)
        first = (self.base["n_blocks"] - 1) * self.base["ns"]
        e = self.pkg.solution_errors_batch(x, self.soln, first=first)
        return {"steps": steps.tolist(), "rel_err": e[:, 0].tolist(), "max_err": e[:, 2].tolist()}

    def close(self):
        self.gn.close(); self.F.close()


def measure(pkg, base, B, steps, runs):
    import torch
    loops = {s: Loop(pkg, base, s, B) for s in ("euler", "cn")}
    row = {"batch": B, "n": base["n"], "n_blocks": base["n_blocks"], "block_size": loops["cn"].F.stats()["block_size"], "steps_timed": steps}
    for s, lp in loops.items():                    # warm-up: one run of each
        lp.run(steps)
        lp.refactor_solve_ms()
    t = {s: {"gn_iter_ms": [], "refactor_solve_ms": []} for s in loops}
    for _ in range(runs):
        for s in ("euler", "cn"):
            t[s]["gn_iter_ms"].append(loops[s].iter_ms(steps))
            t[s]["refactor_solve_ms"].append(loops[s].refactor_solve_ms())
    for s, lp in loops.items():
        r = dict(t[s])
        r["glue_ratio"] = statistics.median(r["gn_iter_ms"]) / statistics.median(r["refactor_solve_ms"])
        r["tangent_ms"], r["tangent_ms_min"] = lp.tangent_ms()
        r["tangent_bytes"] = 8 * B * (lp.tan.nnz + lp.tan.rows + lp.tan.n)
        r["tangent_gbytes_per_s"] = r["tangent_bytes"] / (r["tangent_ms"] * 1e-3) / 1e9
        r["tangent_share_of_iteration"] = 2 * r["tangent_ms"] / statistics.median(r["gn_iter_ms"])
        r.update(lp.to_stop_rule())
        row[s] = r
    e, c = row["euler"]["gn_iter_ms"], row["cn"]["gn_iter_ms"]
    row["cn_median_inside_euler_spread"] = min(e) <= statistics.median(c) <= max(e)
    for lp in loops.values():
        lp.close()
    del loops
    torch.cuda.empty_cache()
    return row


def reference_noise(pkg, base, noise=1e18):
    """Crank-Nicolson at batch 1 with the reference's fem_noise; on NotPositiveDefinite the failing block, then the next powers of ten
    down to the workload's own noise until one factors."""
    import torch
    out = {"fem_noise": noise}
    tries = []
    while noise >= base["noise"]:
        lp = None
        try:
            lp = Loop(pkg, base, "cn", 1, noise=noise)
            r = lp.to_stop_rule()
            tries.append(dict(r, fem_noise=noise, status="ok"))
            break
        except pkg.NotPositiveDefinite as ex:
            tries.append({"fem_noise": noise, "status": "NOT_SPD", "failing_block": ex.info})
        finally:
            if lp is not None:
                lp.close()
            torch.cuda.empty_cache()
        noise /= 10.0
    out["tries"] = tries
    out["largest_power_of_ten_that_factors"] = next((t["fem_noise"] for t in tries if t["status"] == "ok"), None)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nc", type=int, default=1000)
    ap.add_argument("--nt", type=int, default=51)
    ap.add_argument("--nu", type=float, default=0.001)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--skip-reference-noise", action="store_true")
    args = ap.parse_args()
    import __graft_entry__ as g
    pkg = g.load_package()
    base = pkg.workloads.burgers_chen24_batch(args.nc, args.nt, len(AMPS), args.nu, AMPS, order=2)
    out = {"tool": "burgers_cn_latency", "workload": f"burgers_chen24_{args.nc}x{args.nt}", "nu": args.nu, "dt": base["dt"],
           "amps": list(AMPS), "fem_noise": base["noise"], "runs": args.runs, "rows": []}
    for b in args.batches.split(","):
        row = measure(pkg, base, int(b), args.steps, args.runs)
        out["rows"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    if not args.skip_reference_noise:
        out["reference_noise"] = reference_noise(pkg, base)
        print(json.dumps(out["reference_noise"]), file=sys.stderr, flush=True)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
